"""Part 3 (D-NeRF) with the Fourier-coded 8x256 canonical field -- ``canonical_type: nerf``, the reference's default -- and its
direct-time-conditioning ablation (``direct_time_conditioning: true``) as a flat-parameter training engine on fused HIP chains:
the loop body of reference run_part3 (run.py:1040-1222) with NeuralField('part3') (src/core.py:79-146, 233-281).

    standard: every sample of every ray (no occupancy grid for this canonical type) -> t', x' (+ noise) -> deformation chain
    (csrc/p3deform.hip, x_c = x + dx) -> canonical chain at (code(x_c), code(t')) (csrc/p3canon.hip) -> compositing + MSE +
    displacement regulariser + backward (one kernel) -> canonical dgrad + wgrad + d x_c -> deformation chain bwd + wgrad ->
    [temporal / consistency probes] -> [all-reduce] -> ONE global-norm clip + AdamW (one group, cosine schedule).
    direct time conditioning: the canonical chain straight at (code(x), code(t)); no deformation, delta_x = 0.

No torch autograd, torch.optim or library GEMM in the loop.  The flat vector holds the canonical decoder in NeRFDecoder
state-dict order ("decoder.*" or "decoder_direct.*"), followed in standard mode by the deformation MLP.  Under direct time
conditioning the module's unused "decoder.*" and "deform_net.*" get no gradient in the reference (torch.optim.AdamW skips
them); the engine never holds them, so they come back unchanged.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib, flat_params, ops
from . import part3 as p3
from .dynamic_engine import DynamicEngine, clip_adamw_flat, composite_mse_reg_bwd, normsq_flat, sample_inputs
from .flat_engine import render_counted_chain

Tensor = torch.Tensor
P = lambda t: None if t is None else t.data_ptr()
POS_DIM, DIR_DIM = 63, 27


def _dtc(cfg: dict) -> bool:
    return bool(cfg.get("direct_time_conditioning", False))


def time_dim(cfg: dict) -> int:
    """columns of code(t): 1 + 2 L_embed_time (src/embeddings.py:20)"""
    return 1 + 2 * int(cfg.get("L_embed_time", 10))


def supported_nerf(cfg: dict) -> Optional[str]:
    """None if the fused chains are compiled for this configuration (canonical_type nerf, standard or direct time
    conditioning), else the reason they are not, naming the key."""
    if cfg.get("mode") != "part3":
        return f"mode={cfg.get('mode')} (compiled: part3)"
    if cfg.get("canonical_type", "nerf") != "nerf":
        return f"canonical_type={cfg.get('canonical_type')} (compiled: nerf)"
    # (compiled value, NeuralField's default)
    want = {"hidden_dim": (256, 256), "num_layers": (8, 8), "skip_layer": (4, 4), "view_dim": (128, 128), "L_embed_dir": (4, 4),
            "L_embed": (10, 10)}
    if not _dtc(cfg):
        # the deformation chain is compiled for code(x') L 10 + code(t') L 10 = 84 inputs, 128 x 4
        want.update({"L_embed_canon": (10, 10), "L_embed_time": (10, 10), "deform_hidden_dim": (128, 128), "deform_num_layers": (4, 4)})
    for key, (compiled, default) in want.items():
        if cfg.get(key, default) != compiled:
            return f"{key}={cfg.get(key, default)} (compiled: {compiled})"
    if _dtc(cfg):
        lt = cfg.get("L_embed_time", 10)
        if not isinstance(lt, int) or not 0 <= lt <= 10:
            return f"L_embed_time={lt} (compiled: 0..10)"
    return None


def decoder_shapes(prefix: str, code_dim: int):
    """(state-dict key, shape) of NeRFDecoder(pos_dim=code_dim, dir_dim=27) in registration order (src/decoders.py:37-66)"""
    return [(key, shape) for key, _, shape in flat_params.nerf_decoder_table(prefix + ".", code_dim, DIR_DIM)]


def slice_table(cfg: dict):
    """(key, 'net', offset, shape) of every parameter the engine trains, inside its flat vector"""
    table, off = [], 0
    for key, shape in decoder_shapes("decoder_direct" if _dtc(cfg) else "decoder", POS_DIM + time_dim(cfg)):
        table.append((key, "net", off, shape))
        off += math.prod(shape)
    if not _dtc(cfg):
        for key, doff, shape in p3.MODULE_SLICES:
            if key.startswith("deform_net."):
                table.append((key, "net", off + doff - p3.DEFORM0, shape))
    return table


def param_count(cfg: dict) -> int:
    return sum(math.prod(s) for _, _, _, s in slice_table(cfg))


# --------------------------------------------------------------------------------------------------- canonical chain
def canon_pack(params: Tensor, tdim: int, packed: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    if params.numel() != lib.nerf_p3_canon_param_count(tdim) or not params.is_contiguous():
        raise ValueError(f"Part 3 canonical decoder: {lib.nerf_p3_canon_param_count(tdim)} contiguous parameters expected, got {params.numel()}")
    if packed is None:
        packed = torch.empty(lib.nerf_p3_canon_packed_bytes(), dtype=torch.uint8, device=params.device)
    _lib.check(lib.nerf_p3_canon_pack(P(params), int(tdim), P(packed), ops._stream()), "nerf_p3_canon_pack")
    return packed


def canon_workspace_bytes(n: int) -> int:
    return max(_lib.load().nerf_p3_canon_workspace_bytes(n), 256)


def canon_fwd(packed: Tensor, x: Tensor, t: Tensor, dirs: Tensor, workspace: Optional[Tensor] = None):
    """(rgb [n,3], sigma [n]) of the canonical decoder at code(x), code(t), code(dirs); ``workspace``: training forward"""
    lib = _lib.load()
    x, dirs = ops._dev(x, "x"), ops._dev(dirs, "dirs")
    t = ops._dev(t.reshape(-1), "t")
    n = x.shape[0]
    rgb, sigma = torch.empty(n, 3, device=x.device), torch.empty(n, device=x.device)
    if workspace is not None and workspace.numel() < canon_workspace_bytes(n):
        raise ValueError("canon_fwd: workspace too small")
    _lib.check(lib.nerf_p3_canon_fwd(P(packed), P(workspace), P(x), P(t), P(dirs), n, P(rgb), P(sigma), 1 if workspace is not None else 0,
                                     ops._stream()), "nerf_p3_canon_fwd")
    return rgb, sigma


def canon_bwd(packed: Tensor, workspace: Tensor, tdim: int, rgb: Tensor, sigma: Tensor, d_rgb: Tensor, d_sigma: Tensor, grads: Tensor,
              x: Optional[Tensor] = None, d_x: Optional[Tensor] = None) -> None:
    """WRITES the parameter gradients of the last training canon_fwd on ``workspace`` to ``grads``; ADDS d loss / d x to ``d_x``"""
    lib = _lib.load()
    if grads.numel() != lib.nerf_p3_canon_param_count(tdim) or not grads.is_contiguous():
        raise ValueError("canon_bwd: grads must be a contiguous vector of the decoder's parameter count")
    _lib.check(lib.nerf_p3_canon_bwd(P(packed), P(workspace), P(x), P(rgb), P(sigma), P(d_rgb), P(d_sigma), rgb.shape[0], int(tdim),
                                     P(grads), P(d_x), ops._stream()), "nerf_p3_canon_bwd")


# --------------------------------------------------------------------------------------------------- engine
class Part3NerfEngine(DynamicEngine):
    """Flat-parameter training / rendering engine of mode part3 with canonical_type nerf (module docstring)."""
    SLACK = (1.0, 0)                 # exact sizes: n = rays x samples is the same every step
    RENDER_CHUNK = 16384

    def __init__(self, cfg: dict, device: str = "cuda", seed: int = 0, world_size: int = 1):
        why = supported_nerf(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Part 3 canonical chains are not compiled for {why}")
        lib = _lib.load()
        super().__init__(cfg, device, seed, world_size)
        self.dtc = _dtc(cfg)
        self.tdim = time_dim(cfg)
        self.n_canon = int(lib.nerf_p3_canon_param_count(self.tdim))
        self.slices = slice_table(cfg)
        self.n_params = param_count(cfg)
        if self.n_params != self.n_canon + (0 if self.dtc else p3.N_DEFORM):
            raise _lib.NerfHipError(f"libnerf_hip.so reports {self.n_canon} canonical decoder parameters, the slice table "
                                    f"{self.n_params - (0 if self.dtc else p3.N_DEFORM)}")
        if not self.dtc:
            p3._check_count()
        self.net = torch.zeros(self.n_params, device=self.device)
        self._g_net_scalars = torch.zeros(self.n_params + 4, device=self.device)
        self.g_net = self._g_net_scalars[:self.n_params]
        self.state = {"net": (torch.zeros_like(self.net), torch.zeros_like(self.net))}
        self.packed_c = torch.empty(lib.nerf_p3_canon_packed_bytes(), dtype=torch.uint8, device=self.device)
        self.packed_d = None if self.dtc else torch.empty(lib.nerf_p3_deform_packed_bytes(), dtype=torch.uint8, device=self.device)
        if self.dtc:                 # no deformation branch: nothing to regularise, and the noise feeds that branch only
            self.reg_weight = self.std_x = self.std_t = 0.0
        self.last_reg = torch.zeros((), device=self.device)
        self.last_d_dx: Optional[Tensor] = None
        self.repack()

    # -- parameters ------------------------------------------------------------------------------------------
    @property
    def canon_params(self) -> Tensor:
        return self.net[:self.n_canon]

    @property
    def g_canon(self) -> Tensor:
        return self.g_net[:self.n_canon]

    @property
    def deform_params(self) -> Tensor:
        return self.net[self.n_canon:]

    @property
    def g_deform(self) -> Tensor:
        return self.g_net[self.n_canon:]

    def repack(self) -> None:
        canon_pack(self.canon_params, self.tdim, self.packed_c)
        if not self.dtc:
            p3.deform_pack(self.deform_params, self.packed_d)

    def slice_table(self):
        """(key, 'net', offset, shape) of every module parameter the engine trains"""
        return list(self.slices)

    def _deform_ws(self, n: int, which: str = "batch") -> Tensor:
        return self._buf("p3_" + which, p3.deform_workspace_bytes(n))

    def _slots(self, n: int) -> Tensor:
        """every sample is its own row (no compaction)"""
        s = self._ws.get("slots")
        if s is None or s.numel() < n:
            s = self._ws["slots"] = torch.arange(n, dtype=torch.int32, device=self.device)
        return s[:n]

    # -- field -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def field(self, pts: Tensor, dirs: Tensor, t: Tensor):
        """(rgb [n,3], sigma [n], delta_x [n,3]) at points with per-point times, evaluation mode (no noise)"""
        pts, dirs, t = pts.contiguous(), dirs.contiguous(), t.reshape(-1).contiguous()
        if pts.shape[0] == 0:
            return pts.new_zeros(0, 3), pts.new_zeros(0), pts.new_zeros(0, 3)
        if self.dtc:
            rgb, sigma = canon_fwd(self.packed_c, pts, t, dirs)
            return rgb, sigma, torch.zeros_like(pts)
        dx, xc = p3.deform_fwd(self.packed_d, pts, t)
        rgb, sigma = canon_fwd(self.packed_c, xc, t, dirs)
        return rgb, sigma, dx

    def compute_gradients(self, rays_o: Tensor, rays_d: Tensor, target: Tensor, times: Tensor, n_samples: int, u: Optional[Tensor] = None,
                          first_ray: int = 0, bg: Optional[Tensor] = None, sync_grads_async=None, probes=None) -> Tensor:
        """Forward + backward of one batch: fills g_net with the gradient of MSE + deformation_reg_weight * mean(mean_delta_x^2)
        (+ the probe terms) of the LOCAL rays and returns the RGB loss.  ``u`` [R,S]: the stratified jitter (default: torch.rand,
        as render_rays draws it).  ``sync_grads_async(view)``: data-parallel hook (a summing all-reduce; apply_gradients
        divides by the world size)."""
        R, S = rays_o.shape[0], int(n_samples)
        n = R * S
        bg = self.bg if bg is None else bg
        if u is None:
            u = torch.rand(R, S, device=self.device)
        z, pts, dirs = ops.sample_rays(rays_o, rays_d, self.near, self.far, S, u=u, want_points=True)
        slots = self._slots(n)
        self._counter += 1
        self._g_net_scalars.zero_()
        scalars = self._g_net_scalars[self.n_params:]
        loss, reg = scalars[0:1], scalars[1:2]
        x_def, t_def = sample_inputs(slots, pts, times, R, S, self.std_x, self.std_t, self.seed, self._counter, first_ray)
        cws = self._buf("canon", canon_workspace_bytes(n))
        if self.dtc:
            dx = self._ws.get("zeros")
            if dx is None or dx.shape[0] < n:
                dx = self._ws["zeros"] = torch.zeros(n, 3, device=self.device)
            dx = dx[:n]
            xc = pts
        else:
            dws = self._deform_ws(n)
            dx, xc = p3.deform_fwd(self.packed_d, pts, t_def, x_code=x_def, workspace=dws)
        # the canonical decoder sees t' as well (src/core.py:136-139); under direct time conditioning t' = t (no noise)
        rgb, sigma = canon_fwd(self.packed_c, xc, t_def, dirs, workspace=cws)
        d_rgb, d_sigma, d_dx = composite_mse_reg_bwd(rgb, sigma, slots, z, rays_d, bg, target, dx, self.reg_weight, R, S, loss, reg,
                                                     ops.sum_ws(self.device))
        if self.dtc:
            canon_bwd(self.packed_c, cws, self.tdim, rgb, sigma, d_rgb, d_sigma, self.g_canon)
        else:
            # d x_c ADDED to the regulariser's d delta_x (x_c = x + delta_x), then the deformation chain's backward
            canon_bwd(self.packed_c, cws, self.tdim, rgb, sigma, d_rgb, d_sigma, self.g_canon, x=xc, d_x=d_dx)
            self.last_d_dx = d_dx            # d loss / d delta_x the deformation backward consumed (regulariser + d x_c)
            p3.deform_bwd(self.packed_d, dws, d_dx, self.g_deform)
        self.last_reg = reg[0]
        self.last_terms = self._probe_regularisers(probes) if (probes and not self.dtc) else {}
        self._sync_grads(sync_grads_async, self.g_net)
        return loss[0]

    def _probe_regularisers(self, probes: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """temporal smoothness and unsupervised consistency on the deformation chain (part3.deform_probe_regularisers), ADDING
        into g_net"""
        return p3.deform_probe_regularisers(self.cfg, self.packed_d, lambda n: self._deform_ws(n, "probes"), self.g_deform, probes)

    def apply_gradients(self) -> None:
        """ONE global-norm clip over every trained parameter (clip_grad_norm_(model.parameters()), run.py:1174) and AdamW as one
        group with the cosine schedule; after a summing all-reduce the gradient is averaged (1/world)."""
        scale = 1.0 / self.world_size
        normsq_flat(self.net, self.g_net, self.n_params, scale, self._normsq_ws, first=True)
        lr = self.lr()                             # the rate of THIS step: scheduler.step() follows optimizer.step()
        self.step_count += 1
        clip_adamw_flat(self.net, self.g_net, self.state["net"], self.n_params, self.step_count, lr, self.wd, self._normsq_ws, self.max_norm,
                        scale)
        self.repack()

    # -- rendering -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def render_rays(self, rays_o: Tensor, rays_d: Tensor, times: Tensor, n_samples: int, bg: Optional[Tensor] = None):
        """(rgb [R,3], depth [R], acc [R]) with per-ray times [R,1] (or one time), no jitter"""
        R = rays_o.shape[0]
        bg = self.bg if bg is None else bg
        z, pts, dirs = ops.sample_rays(rays_o.contiguous(), rays_d.contiguous(), self.near, self.far, n_samples, want_points=True)
        t = (times.reshape(1, 1).expand(R, 1) if times.numel() == 1 else times.reshape(R, 1)).expand(R, n_samples).reshape(-1).contiguous()
        rgb, sigma, _ = self.field(pts, dirs, t)
        out_rgb, depth, acc, _ = ops.composite(rgb.view(R, n_samples, 3), sigma.view(R, n_samples), z, rays_d.contiguous(), bg)
        return out_rgb, depth, acc

    _chain_ws = None           # render_image_chain: one workspace per (chunk, n_samples)
    _chain_time = None         # ... and the one time word its kernels read

    @torch.no_grad()
    def render_image_chain(self, rays_o: Tensor, rays_d: Tensor, time: Tensor, n_samples: int, chunk: Optional[int] = None,
                           bg: Optional[Tensor] = None) -> Tensor:
        """one view at one time as ONE launch chain (nerf_p3_nerf_render_rays_fwd): the time stays on the device, no time vector, no
        delta_x and no allocation per chunk, the deformation on its scalar-time kernel; the same bits as render_image.  A method of
        its own: render_image(chain=True) keeps raising on this engine, as update_grid(chain=True) / update_grid_chain split on
        Part3InstantEngine."""
        if self._chain_ws is None:
            self._chain_ws, self._chain_time = {}, torch.zeros(1, device=self.device)
        self._chain_time.copy_(time.reshape(1))
        bg = self.bg if bg is None else bg
        return render_counted_chain(
            lambda o, d, chunk, ws: ops.p3_nerf_render_rays_fwd(self.packed_d, self.packed_c, o, d, n_samples, self.near, self.far,
                                                                self._chain_time, bg, chunk, workspace=ws),
            ops.p3_nerf_render_workspace_bytes, self._chain_ws, rays_o, rays_d, n_samples, chunk or self.RENDER_CHUNK, self.device)
