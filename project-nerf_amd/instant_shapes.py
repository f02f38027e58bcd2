"""Instant-NGP (mode part2_instant) at the hash and tiny-MLP shapes the YAML allows, as a flat-parameter training / rendering
engine on the fused HIP chain of csrc/imlp_shapes.hip: the per-step work of reference run_part2_instant (run.py:579-646) around
InstantNeRFDecoder (src/decoders.py:100-162) at n_levels 1..16 (2 features per level), hidden_dim 32 / 64 / 128 and
L_embed_dir 0..4.

    compaction one batch ahead -> hash forward into the chain's workspace -> tiny MLPs with their training images
    (nerf_imlp_shape_fwd) -> indexed compositing + MSE + their backward -> transposed chain, weight gradients by chunk-partial
    MFMA tiles + one ordered reduction (nerf_imlp_shape_bwd) -> counted overwrite-form hash backward -> TV + clip + AdamW on
    the table, clip + AdamW on the nets -> repack; cosine LR on the host.

Everything but the decoder is InstantNgpEngine's step (engine.py), which this class subclasses; the speculative, precounted
and level-major hash backward forms, data parallelism and the sharded optimiser stay with the default shape.  The flat
vector is a non-fused InstantNeRFDecoder's ``sigma_net.params`` and ``color_net.params`` concatenated
(decoders.tiny_mlp_shapes), so checkpoints keep their keys.  The default shape (16, 64, 4) is accepted here too, but run.py
keeps it on InstantNgpEngine.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .decoders import tiny_mlp_init, tiny_mlp_shapes
from .engine import InstantNgpEngine

Tensor = torch.Tensor
P = ops._p

HIDDEN = (32, 64, 128)
MAX_LEVELS, MAX_L_DIR = 16, 4
KEYS = ("n_levels", "n_features_per_level", "hidden_dim", "L_embed_dir", "log2_hashmap_size", "base_resolution", "per_level_scale")


def _shape(cfg: dict) -> Tuple[int, int, int]:
    """(n_levels, hidden_dim, L_embed_dir) as build_instant_field reads them (instant.py)"""
    return int(cfg.get("n_levels", 16)), int(cfg.get("hidden_dim", 64)), int(cfg.get("L_embed_dir", 4))


def supported(cfg: dict) -> Optional[str]:
    """None if the fused shape chain is compiled for this configuration, else the reason it is not."""
    if cfg.get("mode") != "part2_instant":
        return f"mode={cfg.get('mode')} (compiled: part2_instant)"
    for key in KEYS:
        if isinstance(cfg.get(key), (list, tuple)):
            return f"{key}={cfg.get(key)} (compiled: one value)"
    val = {"n_features_per_level": cfg.get("n_features_per_level", 2), "n_levels": cfg.get("n_levels", 16),
           "hidden_dim": cfg.get("hidden_dim", 64), "L_embed_dir": cfg.get("L_embed_dir", 4)}
    for k, v in val.items():
        if not isinstance(v, int) or isinstance(v, bool):
            return f"{k}={v} (compiled: an integer)"
    if val["n_features_per_level"] != 2:
        return f"n_features_per_level={val['n_features_per_level']} (compiled: 2)"
    if not 1 <= val["n_levels"] <= MAX_LEVELS:
        return f"n_levels={val['n_levels']} (compiled: 1..{MAX_LEVELS})"
    if val["hidden_dim"] not in HIDDEN:
        return f"hidden_dim={val['hidden_dim']} (compiled: 32, 64, 128)"
    if not 0 <= val["L_embed_dir"] <= MAX_L_DIR:
        return f"L_embed_dir={val['L_embed_dir']} (compiled: 0..{MAX_L_DIR})"
    if not cfg.get("use_density_grid", True):
        return "use_density_grid=False (compiled: True)"
    return None


def net_shapes(cfg: dict) -> Tuple[List[Tuple[int, int]], List[Tuple[int, int]]]:
    """[out, in] matrices of the sigma-net and of the colour net (decoders.tiny_mlp_shapes, what InstantNeRFDecoder builds)"""
    L, H, Ld = _shape(cfg)
    return tiny_mlp_shapes(2 * L, 16, H, 1), tiny_mlp_shapes(16 + 3 + 6 * Ld, 3, H, 2)


def slice_table(cfg: dict) -> List[Tuple[str, int, Tuple[int, int], Tuple[int, int]]]:
    """(name, offset into the flat vector, padded [out, in] shape, valid (rows, columns)) of every weight matrix, in the order
    decoder.sigma_net.params | decoder.color_net.params"""
    L, H, Ld = _shape(cfg)
    s, c = net_shapes(cfg)
    valid = [(H, 2 * L), (16, H), (H, 16 + 3 + 6 * Ld), (H, H), (3, H)]
    names = ["sigma_net.0", "sigma_net.1", "color_net.0", "color_net.1", "color_net.2"]
    table, off = [], 0
    for name, shape, v in zip(names, s + c, valid):
        table.append((name, off, shape, v))
        off += shape[0] * shape[1]
    return table


def param_count(cfg: dict) -> int:
    name, off, shape, _ = slice_table(cfg)[-1]
    return off + shape[0] * shape[1]


def sigma_count(cfg: dict) -> int:
    return slice_table(cfg)[2][1]


def flatten(cfg: dict, sigma_params: Tensor, color_params: Tensor) -> Tensor:
    """the module's two ``params`` tensors -> the engine's vector"""
    flat = torch.cat([sigma_params.detach().float().reshape(-1), color_params.detach().float().reshape(-1)])
    if flat.numel() != param_count(cfg):
        raise ValueError(f"Instant shape engine: {param_count(cfg)} parameters expected, got {flat.numel()}")
    return flat


def unflatten(cfg: dict, flat: Tensor) -> Dict[str, Tensor]:
    """the engine's vector -> views under the module's state-dict keys"""
    n = sigma_count(cfg)
    return {"decoder.sigma_net.params": flat[:n], "decoder.color_net.params": flat[n:]}


class InstantShapeEngine(InstantNgpEngine):
    """InstantNgpEngine's step with the tiny MLPs of csrc/imlp_shapes.hip (module docstring); one rank, counted hash backward."""

    def __init__(self, cfg: Optional[dict] = None, device: str = "cuda", seed: int = 0, world_size: int = 1):
        cfg = dict(cfg or {})
        cfg.setdefault("mode", "part2_instant")
        if world_size != 1:
            raise NotImplementedError("the Instant shape engine runs on one rank (data parallelism: the default shape's engine)")
        # the forms built around imlp.hip's level-major / amax outputs stay with the default shape
        cfg["speculative_hash_backward"] = False
        cfg["precount"] = False
        self.cfg = cfg
        super().__init__(cfg, device=device, seed=seed, world_size=1)

    # ---- the decoder's shape-specific pieces
    def _check_shape(self, cfg: dict) -> None:
        why = supported(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Instant shape chain is not compiled for {why}")
        self.shape = _shape(cfg)
        n = ops._lib.load().nerf_imlp_shape_param_count(*self.shape)
        if n != param_count(cfg):
            raise ops._lib.NerfHipError(f"libnerf_hip.so reports {n} tiny-MLP parameters, this binding expects {param_count(cfg)}")

    def _init_net(self, g: torch.Generator) -> Tensor:
        # decoders.tiny_mlp_init draws from torch's global generator: seed it from this engine's, restore it afterwards
        L, H, Ld = self.shape
        state = torch.random.get_rng_state()
        try:
            torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
            return torch.cat([tiny_mlp_init(2 * L, 16, H, 1), tiny_mlp_init(16 + 3 + 6 * Ld, 3, H, 2)])
        finally:
            torch.random.set_rng_state(state)

    def _pack(self) -> None:
        lib = ops._lib.load()
        if self.packed is None:
            self.packed = torch.empty(lib.nerf_imlp_shape_packed_bytes(*self.shape), device=self.device, dtype=torch.uint8)
        ops._lib.check(lib.nerf_imlp_shape_pack(P(self.net), *self.shape, P(self.packed), ops._stream()), "nerf_imlp_shape_pack")

    def set_net(self, sigma_params: Tensor, color_params: Tensor) -> None:
        """weights of a non-fused InstantNeRFDecoder (its two ``params`` tensors) -> the engine, repacked"""
        with torch.no_grad():
            self.net.copy_(flatten(self.cfg, sigma_params, color_params).to(self.device))
        self._pack()

    def _field(self, pts: Tensor, dirs: Tensor, train: bool, hist_ws: Optional[Tensor] = None):
        if hist_ws is not None:
            raise NotImplementedError("the precounted hash backward stays with the default shape")
        lib = ops._lib.load()
        n = pts.shape[0]
        ws = torch.empty(lib.nerf_imlp_shape_workspace_bytes(n, *self.shape), device=self.device, dtype=torch.uint8)
        nat = ws[lib.nerf_imlp_shape_hash_operand_offset(n, *self.shape):]
        ops.hash_encode_fwd(pts, self._gather_table(), self.levels, self.bound, want_f32=False, out_nat=nat)
        rgb, sigma = torch.empty(n, 3, device=self.device), torch.empty(n, device=self.device)
        dirs = dirs if dirs.is_contiguous() else dirs.contiguous()
        ops._lib.check(lib.nerf_imlp_shape_fwd(P(self.packed), P(ws), P(dirs), n, *self.shape, P(rgb), P(sigma), 1 if train else 0,
                                               ops._stream()), "nerf_imlp_shape_fwd")
        return rgb, sigma, ws

    def _decoder_bwd(self, ws: Tensor, rgb: Tensor, sigma: Tensor, d_rgb: Tensor, d_sigma: Tensor, n: int, d_feat: Tensor) -> None:
        ops._lib.check(ops._lib.load().nerf_imlp_shape_bwd(P(self.packed), P(ws), P(rgb), P(sigma), P(d_rgb), P(d_sigma), n, *self.shape,
                                                           P(self.g_net), P(d_feat), ops._stream()), "nerf_imlp_shape_bwd")

    def _render_image_chain(self, rays_o: Tensor, rays_d: Tensor, n_samples: int, chunk: int) -> Tensor:
        raise NotImplementedError("render_image(chain=True): the evaluation launch chain (nerf_instant_render_rays_fwd) is wired for the "
                                  "default shape's decoder kernel; the shape engine's chain is another kernel -- use chain=False")

    def _update_grid_chain(self) -> float:
        raise NotImplementedError("update_grid(chain=True): the density-only refresh chain (nerf_instant_grid_update) is wired for the "
                                  "default shape's sigma-net kernel; the shape engine's chain is another kernel -- use chain=False")

    def enable_sharded_optimizer(self, rank: int) -> None:
        raise NotImplementedError("the sharded optimiser stays with the default shape's engine")
