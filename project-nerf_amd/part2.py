"""Vanilla NeRF (mode part2_nerf) at a non-default decoder shape as a flat-parameter training / rendering engine on one fused HIP
chain: the loop body of reference run_part2 (run.py:312-338) and render_image (src/renderer.py:387-418) with
NeuralField('part2_nerf') (src/core.py:36-55, src/decoders.py:29-87).

    sample -> decoder forward with its training images (csrc/p2chain.hip) -> compositing + MSE + their backward
    (ops.composite_mse_bwd, the loss an ordered sum) -> transposed chain -> weight gradients by chunk-partial MFMA tiles + one
    ordered reduction -> Adam (ops.adam_step, torch.optim.Adam's defaults) -> repack.

No torch autograd, torch.optim or library GEMM in the step.  The flat vector is the module's state dict concatenated
(decoder.pts_layers.*, sigma_layer, feature_layer, view_layer, rgb_layer), so checkpoints keep the reference's keys.  The
default shape (256 x 8, skip 4, view 128) is accepted here too, but run.py keeps it on engine.VanillaNerfEngine.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, flat_params, ops
from .flat_engine import FlatAdamEngine, LapSlots, render_chunks

Tensor = torch.Tensor
P = ops._p

HIDDEN = (64, 128, 256)
VIEW = (64, 128)
MIN_LAYERS, MAX_LAYERS, MAX_L, MAX_L_DIR = 2, 8, 10, 4


def _shape(cfg: dict) -> Tuple[int, int, int, int, int, int]:
    """(hidden_dim, num_layers, skip_layer, view_dim, L_embed, L_embed_dir) as NeuralField reads them (src/core.py:36-55)"""
    return (int(cfg.get("hidden_dim", 256)), int(cfg.get("num_layers", 8)), int(cfg.get("skip_layer", 4)), int(cfg.get("view_dim", 128)),
            int(cfg.get("L_embed", 0)), int(cfg.get("L_embed_dir", 4)) if cfg.get("use_viewdirs", True) else 0)


def supported(cfg: dict) -> Optional[str]:
    """None if the fused chain is compiled for this configuration, else the reason it is not."""
    if cfg.get("mode") != "part2_nerf":
        return f"mode={cfg.get('mode')} (compiled: part2_nerf)"
    keys = ("hidden_dim", "num_layers", "skip_layer", "view_dim", "L_embed", "L_embed_dir")
    for key in keys + ("use_positional_encoding", "use_viewdirs"):
        if isinstance(cfg.get(key), (list, tuple)):
            return f"{key}={cfg.get(key)} (compiled: one value)"
    if not cfg.get("use_positional_encoding", True):
        return "use_positional_encoding=False (compiled: True)"
    if not cfg.get("use_viewdirs", True):
        return "use_viewdirs=False (compiled: True)"
    get = {"hidden_dim": 256, "num_layers": 8, "skip_layer": 4, "view_dim": 128, "L_embed": 0, "L_embed_dir": 4}
    val = {k: cfg.get(k, d) for k, d in get.items()}
    for k, v in val.items():
        if not isinstance(v, int) or isinstance(v, bool):
            return f"{k}={v} (compiled: an integer)"
    if val["hidden_dim"] not in HIDDEN:
        return f"hidden_dim={val['hidden_dim']} (compiled: 64, 128, 256)"
    if not MIN_LAYERS <= val["num_layers"] <= MAX_LAYERS:
        return f"num_layers={val['num_layers']} (compiled: {MIN_LAYERS}..{MAX_LAYERS})"
    if val["skip_layer"] == 0:
        return "skip_layer=0 (compiled: 1..num_layers-1, or no skip)"
    if val["view_dim"] not in VIEW:
        return f"view_dim={val['view_dim']} (compiled: 64, 128)"
    if not 1 <= val["L_embed"] <= MAX_L:
        return f"L_embed={val['L_embed']} (compiled: 1..{MAX_L})"
    if not 0 <= val["L_embed_dir"] <= MAX_L_DIR:
        return f"L_embed_dir={val['L_embed_dir']} (compiled: 0..{MAX_L_DIR})"
    return None


def slice_table(cfg: dict) -> flat_params.Table:
    """(state-dict key, offset into the flat vector, shape) of every parameter of NeuralField(cfg), in state-dict order"""
    H, layers, skip, V, L, Ld = _shape(cfg)
    return flat_params.nerf_decoder_table("decoder.", 3 + 6 * L, 3 + 6 * Ld, H, layers, skip, V)


param_count, flatten, unflatten, default_init = flat_params.bind(slice_table)       # each takes cfg first


class Part2Engine(FlatAdamEngine):
    """Flat-parameter training / rendering engine of mode part2_nerf on the fused chain of csrc/p2chain.hip (module docstring)."""
    RING = 1024

    def __init__(self, cfg: dict, device: str = "cuda", params: Optional[Tensor] = None, lr: float = 5e-4, near: float = 2.0,
                 far: float = 6.0, white_bkgd: bool = True, seed: int = 0):
        why = supported(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Part 2 chain is not compiled for {why}")
        self.cfg = dict(cfg)
        self.shape = _shape(cfg)
        lib = _lib.load()
        super().__init__("Part 2", slice_table(cfg), lib.nerf_p2_param_count(*self.shape), lib.nerf_p2_packed_bytes(*self.shape),
                         default_init(cfg, seed) if params is None else params, device, lr)
        self.near, self.far = float(near), float(far)
        self.bg = (torch.ones(3) if white_bkgd else torch.zeros(3)).to(self.device)
        self._losses = LapSlots(torch.zeros(1, self.RING, device=self.device))       # one zeroed slot per step, cleared once per lap
        self.repack()

    # -- weights -------------------------------------------------------------------------------------------------
    def repack(self) -> None:
        _lib.check(_lib.load().nerf_p2_pack(P(self.params), *self.shape, P(self.packed), ops._stream()), "nerf_p2_pack")

    def _workspace_bytes(self, n: int) -> int:
        return _lib.load().nerf_p2_workspace_bytes(n, *self.shape)

    # -- field ---------------------------------------------------------------------------------------------------
    def _forward(self, o: Tensor, d: Tensor, z: Optional[Tensor], n: int, n_samples: int, train: bool) -> Tuple[Tensor, Tensor]:
        rgb, sigma = torch.empty(n, 3, device=self.device), torch.empty(n, device=self.device)
        lib = _lib.load()
        if train:
            _lib.check(lib.nerf_p2_fwd_train(P(self.packed), P(self._workspace(n)), P(o), P(d), P(z), n, n_samples, *self.shape, P(rgb),
                                             P(sigma), ops._stream()), "nerf_p2_fwd_train")
        else:
            _lib.check(lib.nerf_p2_fwd(P(self.packed), P(o), P(d), P(z), n, n_samples, *self.shape, P(rgb), P(sigma), ops._stream()),
                       "nerf_p2_fwd")
        return rgb, sigma

    def field(self, pts: Tensor, dirs: Tensor, train: bool = False) -> Tuple[Tensor, Tensor]:
        """rgb [n,3], sigma [n] at pts [n,3] with view directions dirs [n,3] (encoded as given).  ``train``: keeps the layer
        images for a following ``backward``."""
        pts, dirs = ops._dev(pts, "pts"), ops._dev(dirs, "dirs")
        if pts.dim() != 2 or pts.shape[1] != 3 or dirs.shape != pts.shape:
            raise ValueError(f"pts [n,3] and dirs [n,3] expected, got {tuple(pts.shape)} and {tuple(dirs.shape)}")
        return self._forward(pts, dirs, None, pts.shape[0], 0, train)

    def field_from_rays(self, rays_o: Tensor, rays_d: Tensor, z: Tensor, train: bool = False) -> Tuple[Tensor, Tensor]:
        """rgb [R*S,3], sigma [R*S] at x = o + d z with v = d / |d|, formed in registers"""
        rays_o, rays_d, z = ops._dev(rays_o, "rays_o"), ops._dev(rays_d, "rays_d"), ops._dev(z, "z")
        R, S = z.shape
        if rays_o.shape != (R, 3) or rays_d.shape != (R, 3):
            raise ValueError(f"rays_o / rays_d [{R},3] expected, got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
        return self._forward(rays_o, rays_d, z, R * S, S, train)

    def backward(self, rgb: Tensor, sigma: Tensor, d_rgb: Tensor, d_sigma: Tensor) -> Tensor:
        """``grads`` from d loss / d rgb [n,3], d sigma [n] and the outputs of the last training forward"""
        n = sigma.numel()
        if n > 0:
            _lib.check(_lib.load().nerf_p2_bwd(P(self.packed), P(self._workspace(n)), P(ops._dev(rgb, "rgb")), P(ops._dev(sigma, "sigma")),
                                               P(ops._dev(d_rgb, "d_rgb")), P(ops._dev(d_sigma, "d_sigma")), n, *self.shape, P(self.grads),
                                               ops._stream()), "nerf_p2_bwd")
        return self.grads

    # -- step (reference run.py:314-338) -------------------------------------------------------------------------
    def compute_gradients(self, rays_o: Tensor, rays_d: Tensor, target: Tensor, n_samples: int = 64, u: Optional[Tensor] = None,
                          z: Optional[Tensor] = None) -> Tensor:
        """Fills ``grads`` with the gradient of mean((render(rays) - target)^2) and returns the loss (a device scalar).
        ``z`` [R, n_samples]: depths the caller already has; otherwise stratified with jitter ``u`` (or torch.rand)."""
        R = rays_o.shape[0]
        if R == 0:
            raise ValueError("empty batch")
        if z is None:
            if u is None:
                u = torch.rand(R, n_samples, device=self.device)
            z = ops.sample_rays(rays_o, rays_d, self.near, self.far, n_samples, u=u)
        n_samples = z.shape[1]
        rgb, sigma = self.field_from_rays(rays_o, rays_d, z, train=True)
        (loss,) = self._losses.take()
        d_rgb, d_sigma, _ = ops.composite_mse_bwd(rgb.view(R, n_samples, 3), sigma.view(R, n_samples), z, rays_d, self.bg, target, loss)
        self.backward(rgb, sigma, d_rgb.view(-1, 3), d_sigma.view(-1))
        return LapSlots.keep(loss)   # a copy: the ring is cleared every RING steps

    # -- inference (reference render_image, src/renderer.py:387-418) ---------------------------------------------
    @torch.no_grad()
    def render_rays(self, rays_o: Tensor, rays_d: Tensor, n_samples: int, u: Optional[Tensor] = None):
        rays_o, rays_d = ops._dev(rays_o, "rays_o"), ops._dev(rays_d, "rays_d")
        R = rays_o.shape[0]
        z = ops.sample_rays(rays_o, rays_d, self.near, self.far, n_samples, u=u)
        rgb, sigma = self.field_from_rays(rays_o, rays_d, z)
        c, depth, acc, _ = ops.composite(rgb.view(R, n_samples, 3), sigma.view(R, n_samples), z, rays_d, self.bg)
        return c, depth, acc

    @torch.no_grad()
    def render_image(self, rays_o: Tensor, rays_d: Tensor, n_samples: int, chunk: int = 65536) -> Tensor:
        return render_chunks(lambda o, d: self.render_rays(o, d, n_samples), rays_o, rays_d, chunk, self.device)
