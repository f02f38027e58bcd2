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

import math
from typing import Dict, List, Optional, Tuple

import torch

Tensor = torch.Tensor
P = lambda t: None if t is None else t.data_ptr()

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


def slice_table(cfg: dict) -> List[Tuple[str, int, Tuple[int, ...]]]:
    """(state-dict key, offset into the flat vector, shape) of every parameter of NeuralField(cfg), in state-dict order"""
    H, layers, skip, V, L, Ld = _shape(cfg)
    C, D = 3 + 6 * L, 3 + 6 * Ld
    shapes = []
    for i in range(layers):
        k = C if i == 0 else H
        if i == skip:
            k += C
        shapes.append((f"pts_layers.{i}", (H, k)))
    shapes += [("sigma_layer", (1, H)), ("feature_layer", (H, H)), ("view_layer", (V, H + D)), ("rgb_layer", (3, V))]
    table, off = [], 0
    for name, shape in shapes:
        for key, shp in ((f"decoder.{name}.weight", shape), (f"decoder.{name}.bias", shape[:1])):
            table.append((key, off, shp))
            off += math.prod(shp)
    return table


def param_count(cfg: dict) -> int:
    key, off, shape = slice_table(cfg)[-1]
    return off + math.prod(shape)


def flatten(cfg: dict, state: Dict[str, Tensor]) -> Tensor:
    return torch.cat([state[k].detach().float().reshape(-1) for k, _, _ in slice_table(cfg)])


def unflatten(cfg: dict, flat: Tensor) -> Dict[str, Tensor]:
    return {k: flat[off:off + math.prod(shape)].view(shape) for k, off, shape in slice_table(cfg)}


def default_init(cfg: dict, seed: int = 0) -> Tensor:
    """nn.Linear's default initialisation (weights and biases uniform in +-1/sqrt(fan_in)) of every layer, flat"""
    g = torch.Generator().manual_seed(seed)
    flat = torch.empty(param_count(cfg))
    fan_in = {k: shape[1] for k, _, shape in slice_table(cfg) if k.endswith("weight")}
    for key, off, shape in slice_table(cfg):
        bound = 1.0 / math.sqrt(fan_in[key.replace("bias", "weight")])       # a bias takes its layer's fan-in
        n = math.prod(shape)
        flat[off:off + n] = (torch.rand(n, generator=g) * 2 - 1) * bound
    return flat


class Part2Engine:
    """Flat-parameter training / rendering engine of mode part2_nerf on the fused chain of csrc/p2chain.hip (module docstring)."""
    RING = 1024

    def __init__(self, cfg: dict, device: str = "cuda", params: Optional[Tensor] = None, lr: float = 5e-4, near: float = 2.0,
                 far: float = 6.0, white_bkgd: bool = True, seed: int = 0):
        why = supported(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Part 2 chain is not compiled for {why}")
        from . import _lib
        self.cfg = dict(cfg)
        self.shape = _shape(cfg)
        self.device = torch.device(device)
        lib = _lib.load()
        n = lib.nerf_p2_param_count(*self.shape)
        if n != param_count(cfg):
            raise _lib.NerfHipError(f"libnerf_hip.so reports {n} Part 2 parameters, this binding expects {param_count(cfg)}")
        flat = default_init(cfg, seed) if params is None else params.detach().float().reshape(-1)
        if flat.numel() != n:
            raise ValueError(f"Part 2 engine: {n} parameters expected, got {flat.numel()}")
        self.params = flat.to(self.device).contiguous().clone()
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.packed = torch.empty(lib.nerf_p2_packed_bytes(*self.shape), dtype=torch.uint8, device=self.device)
        self.lr, self.near, self.far = float(lr), float(near), float(far)
        self.bg = (torch.ones(3) if white_bkgd else torch.zeros(3)).to(self.device)
        self.step_count = 0
        self._ws: Optional[Tensor] = None
        self._losses = torch.zeros(self.RING, device=self.device)       # one zeroed slot per step, cleared once per lap
        self._calls = 0
        self.repack()

    # -- weights -------------------------------------------------------------------------------------------------
    def repack(self) -> None:
        from . import _lib, ops
        _lib.check(_lib.load().nerf_p2_pack(P(self.params), *self.shape, P(self.packed), ops._stream()), "nerf_p2_pack")

    def load_from_model(self, model) -> None:
        with torch.no_grad():
            self.params.copy_(flatten(self.cfg, model.state_dict()).to(self.device))
        self.repack()

    def copy_to_model(self, model) -> None:
        state = model.state_dict()                     # references to the module's tensors (buffers such as freq_bands stay)
        with torch.no_grad():
            for k, v in unflatten(self.cfg, self.params).items():
                state[k].copy_(v)

    def state_dict(self, prefix: str = "decoder.") -> Dict[str, Tensor]:
        return {prefix + k[len("decoder."):]: v.clone() for k, v in unflatten(self.cfg, self.params).items()}

    def _workspace(self, n: int) -> Tensor:
        from . import _lib
        need = _lib.load().nerf_p2_workspace_bytes(n, *self.shape)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)        # grow-only
        return self._ws

    # -- field ---------------------------------------------------------------------------------------------------
    def _forward(self, o: Tensor, d: Tensor, z: Optional[Tensor], n: int, n_samples: int, train: bool) -> Tuple[Tensor, Tensor]:
        from . import _lib, ops
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
        from . import ops
        pts, dirs = ops._dev(pts, "pts"), ops._dev(dirs, "dirs")
        if pts.dim() != 2 or pts.shape[1] != 3 or dirs.shape != pts.shape:
            raise ValueError(f"pts [n,3] and dirs [n,3] expected, got {tuple(pts.shape)} and {tuple(dirs.shape)}")
        return self._forward(pts, dirs, None, pts.shape[0], 0, train)

    def field_from_rays(self, rays_o: Tensor, rays_d: Tensor, z: Tensor, train: bool = False) -> Tuple[Tensor, Tensor]:
        """rgb [R*S,3], sigma [R*S] at x = o + d z with v = d / |d|, formed in registers"""
        from . import ops
        rays_o, rays_d, z = ops._dev(rays_o, "rays_o"), ops._dev(rays_d, "rays_d"), ops._dev(z, "z")
        R, S = z.shape
        if rays_o.shape != (R, 3) or rays_d.shape != (R, 3):
            raise ValueError(f"rays_o / rays_d [{R},3] expected, got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
        return self._forward(rays_o, rays_d, z, R * S, S, train)

    def backward(self, rgb: Tensor, sigma: Tensor, d_rgb: Tensor, d_sigma: Tensor) -> Tensor:
        """``grads`` from d loss / d rgb [n,3], d sigma [n] and the outputs of the last training forward"""
        from . import _lib, ops
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
        from . import ops
        R = rays_o.shape[0]
        if R == 0:
            raise ValueError("empty batch")
        if z is None:
            if u is None:
                u = torch.rand(R, n_samples, device=self.device)
            z = ops.sample_rays(rays_o, rays_d, self.near, self.far, n_samples, u=u)
        n_samples = z.shape[1]
        rgb, sigma = self.field_from_rays(rays_o, rays_d, z, train=True)
        slot = self._calls % self.RING
        self._calls += 1
        if slot == 0:
            self._losses.zero_()
        loss = self._losses[slot:slot + 1]
        d_rgb, d_sigma, _ = ops.composite_mse_bwd(rgb.view(R, n_samples, 3), sigma.view(R, n_samples), z, rays_d, self.bg, target, loss)
        self.backward(rgb, sigma, d_rgb.view(-1, 3), d_sigma.view(-1))
        return loss[0].clone()       # a copy: the ring is cleared every RING steps

    def apply_gradients(self) -> None:
        """torch.optim.Adam's defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay), then the fragment image again"""
        from . import ops
        self.step_count += 1
        ops.adam_step(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr)
        self.repack()

    def train_step(self, rays_o: Tensor, rays_d: Tensor, target: Tensor, n_samples: int = 64, u: Optional[Tensor] = None,
                   z: Optional[Tensor] = None) -> Tensor:
        loss = self.compute_gradients(rays_o, rays_d, target, n_samples, u=u, z=z)
        self.apply_gradients()
        return loss

    # -- inference (reference render_image, src/renderer.py:387-418) ---------------------------------------------
    @torch.no_grad()
    def render_rays(self, rays_o: Tensor, rays_d: Tensor, n_samples: int, u: Optional[Tensor] = None):
        from . import ops
        rays_o, rays_d = ops._dev(rays_o, "rays_o"), ops._dev(rays_d, "rays_d")
        R = rays_o.shape[0]
        z = ops.sample_rays(rays_o, rays_d, self.near, self.far, n_samples, u=u)
        rgb, sigma = self.field_from_rays(rays_o, rays_d, z)
        c, depth, acc, _ = ops.composite(rgb.view(R, n_samples, 3), sigma.view(R, n_samples), z, rays_d, self.bg)
        return c, depth, acc

    @torch.no_grad()
    def render_image(self, rays_o: Tensor, rays_d: Tensor, n_samples: int, chunk: int = 65536) -> Tensor:
        shape = rays_o.shape[:-1]
        o, d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
        out = torch.empty(o.shape[0], 3, device=self.device)
        for i in range(0, o.shape[0], chunk):
            out[i:i + chunk] = self.render_rays(o[i:i + chunk], d[i:i + chunk], n_samples)[0]
        return out.view(*shape, 3)
