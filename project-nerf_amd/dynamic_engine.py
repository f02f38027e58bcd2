"""What the flat-parameter engines of the dynamic modes share on the host side (part4.DualHashEngine, part3.Part3InstantEngine,
part3_nerf.Part3NerfEngine): the common configuration and state, the cosine schedule, the grow-only byte buffers, the module <->
flat copies over a slice table, train_step, the image loop, the occupancy-grid plumbing of the two grid engines, and the
kernel-call idioms every step repeats (t' / x' of the samples, fused compositing + loss + regulariser + backward, the squared
norm and clip + AdamW of a flat buffer without a TV term).  Each engine keeps its own parameter layout, repack, field,
compute_gradients and apply_gradients: that is where they differ."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib, ops
from .flat_engine import cosine_lr, render_chunks

Tensor = torch.Tensor
P = lambda t: None if t is None else t.data_ptr()


# --------------------------------------------------------------------------------------------------- kernel-call idioms
def sample_inputs(slots: Optional[Tensor], pts: Tensor, times: Tensor, n_rays: int, n_samples: int, std_x: float = 0.0,
                  std_t: float = 0.0, seed: int = 0, counter: int = 0, first_ray: int = 0):
    """(x' [n,3] or None, t' [n]) of the compacted samples (``n_samples`` > 0: ``times`` per ray) or of plain points
    (``n_samples`` == 0: ``times`` per point)."""
    lib = _lib.load()
    n = pts.shape[0]
    t_def = torch.empty(n, device=pts.device)
    x_def = torch.empty(n, 3, device=pts.device) if std_x > 0.0 else None
    _lib.check(lib.nerf_p4_sample_inputs(P(slots), P(pts), P(ops._dev(times.reshape(-1), "times")), n_rays, n_samples, float(std_x),
                                         float(std_t), int(seed), int(counter) & 0xFFFFFF, int(first_ray), P(x_def), P(t_def),
                                         ops._stream()), "nerf_p4_sample_inputs")
    return x_def, t_def


def composite_mse_reg_bwd(rgb: Tensor, sigma: Tensor, slots: Tensor, z: Tensor, rays_d: Tensor, bg: Tensor, target: Tensor, dx: Tensor,
                          reg_weight: float, n_rays: int, n_samples: int, loss: Tensor, reg: Tensor, sum_ws: Tensor):
    """Compositing of the indexed samples onto ``bg`` + MSE against ``target`` + reg_weight * mean(mean_delta_x^2) and their
    backward in one kernel: the RGB loss and the WEIGHTED regulariser (reg_weight * mean(mean_delta_x^2), as the header states) are ADDED to the one-element ``loss`` / ``reg``
    (``sum_ws``: ops.sum_ws of the engine's device, scratch of their ordered sums); returns (d_rgb [n,3], d_sigma [n], d_dx [n,3])."""
    d_rgb, d_sigma, d_dx = torch.empty_like(rgb), torch.empty_like(sigma), torch.empty_like(dx)
    _lib.check(_lib.load().nerf_composite_mse_reg_bwd(P(rgb), P(sigma), P(slots), P(z), P(rays_d), P(bg), 1, P(target), 1.0 / (3 * n_rays),
                                                      P(dx), reg_weight / (3 * n_rays), n_rays, n_samples, None, None, P(loss), P(reg),
                                                      P(d_rgb), P(d_sigma), P(d_dx), P(sum_ws), ops._stream()),
               "nerf_composite_mse_reg_bwd")
    return d_rgb, d_sigma, d_dx


def normsq_flat(params: Tensor, grads: Tensor, n: int, scale: float, normsq: Tensor, first: bool) -> None:
    """squared norm of ``scale`` * grads (no TV term) into the workspace ``normsq``: the step's ``first`` call STORES it (no
    zeroing launch), later calls add"""
    ops.tv_normsq_codes(params, grads, n, normsq, grad_scale=scale, accumulate=not first)


def clip_adamw_flat(params: Tensor, grads: Tensor, state, n: int, step: int, lr: float, wd: float, normsq: Tensor, max_norm: float,
                    scale: float, solo: int = 0, solo_lr: float = 0.0) -> None:
    """global-norm clip (the finished squared norm in ``normsq``) + AdamW of a flat network buffer with no TV term and no fp16
    copy; ``state`` = (exp_avg, exp_avg_sq).  ``solo_lr`` != 0: element ``solo`` steps at its own rate."""
    ops.adamw_clip_step_tv(params, grads, *state, n, step, lr, normsq, weight_decay=wd, max_norm=max_norm, grad_scale=scale,
                           lr_split=(solo, solo_lr))


def wait_all(handles) -> None:
    """the tail of the data-parallel gradient hook: wait on what ``sync_grads_async`` returned (None: nothing to wait on)"""
    for h in handles:
        if h is not None:
            h.wait()


# --------------------------------------------------------------------------------------------------- engines
class DynamicEngine:
    """State and methods common to the three engines.  A subclass sets its parameter buffers (``net``, ``g_net``, tables),
    defines slice_table, repack, field, render_rays, compute_gradients and apply_gradients, and calls repack() last in __init__."""
    REG_WEIGHT = 1e-4                # default of deformation_reg_weight
    SLACK = (1.25, 0)                # a grow-only buffer is allocated with need * SLACK[0] + SLACK[1] bytes
    RENDER_CHUNK = 65536             # rays per render_rays call of render_image

    def __init__(self, cfg: dict, device: str, seed: int, world_size: int):
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        self.seed, self.world_size = int(seed), int(world_size)
        self.near, self.far = float(cfg.get("near", 2.0)), float(cfg.get("far", 6.0))
        self.lr0, self.eta_min = float(cfg.get("learning_rate", 5e-4)), float(cfg.get("eta_min", 1e-4))
        self.t_max = int(cfg.get("train_iters", 20000))
        self.wd = float(cfg.get("weight_decay", 1e-5))
        self.max_norm = float(cfg.get("max_grad_norm", 1.0))
        self.reg_weight = float(cfg.get("deformation_reg_weight", self.REG_WEIGHT))
        noisy = bool(cfg.get("use_coord_noise", False))
        self.std_x = float(cfg.get("coord_noise_std", 0.005)) if noisy else 0.0
        self.std_t = float(cfg.get("time_noise_std", 0.02)) if noisy else 0.0
        self.bg = (torch.ones(3) if cfg.get("white_bkgd", True) else torch.zeros(3)).to(self.device)
        self.step_count = 0
        self._normsq_ws = ops.normsq_ws(self.device)
        self._ws: Dict[str, Tensor] = {}
        self._counter = 0
        self.last_terms: Dict[str, Tensor] = {}

    def lr(self, mult: float = 1.0) -> float:
        """CosineAnnealingLR of a group whose initial rate is mult * learning_rate (run.py:1016-1021, 1684-1743)"""
        return cosine_lr(self.lr0 * mult, self.eta_min, self.step_count, self.t_max)

    def _buf(self, name: str, nbytes: int) -> Tensor:
        """ONE grow-only byte buffer per use: the active-point count changes almost every step, a buffer per count would churn
        hundreds of MB through the allocator"""
        if name not in self._ws or self._ws[name].numel() < nbytes:
            self._ws.pop(name, None)                         # release before growing
            self._ws[name] = torch.empty(int(nbytes * self.SLACK[0]) + self.SLACK[1], dtype=torch.uint8, device=self.device)
        return self._ws[name]

    # -- module <-> flat buffers ---------------------------------------------------------------------------------
    def _copy_slices(self, model, to_model: bool) -> None:
        """walks slice_table(): (key, attribute holding the flat buffer, offset, shape or None for the whole parameter)"""
        sd = dict(model.named_parameters())
        with torch.no_grad():
            for key, kind, off, shape in self.slice_table():
                cnt = sd[key].numel() if shape is None else math.prod(shape)
                flat = getattr(self, kind)[off:off + cnt]
                if to_model:
                    sd[key].copy_(flat.view(sd[key].shape))
                else:
                    flat.copy_(sd[key].reshape(-1))

    def load_from_model(self, model) -> None:
        self._copy_slices(model, to_model=False)
        self.repack()

    def copy_to_model(self, model) -> None:
        """the trained parameters only: every other parameter of the module is left as it is"""
        self._copy_slices(model, to_model=True)

    # -- step ----------------------------------------------------------------------------------------------------
    def train_step(self, rays_o, rays_d, target, times, n_samples, *args, **kwargs) -> Tensor:
        """compute_gradients (further arguments are its own) then apply_gradients; returns the RGB loss"""
        loss = self.compute_gradients(rays_o, rays_d, target, times, n_samples, *args, **kwargs)
        self.apply_gradients()
        return loss

    @staticmethod
    def _sync_grads(sync_grads_async, *views) -> None:
        """data-parallel hook: start the collective of every gradient view, then wait for all of them"""
        if sync_grads_async is not None:
            wait_all([sync_grads_async(v) for v in views])

    # -- rendering -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def render_image(self, rays_o: Tensor, rays_d: Tensor, time: Tensor, n_samples: int, chunk: Optional[int] = None,
                     bg: Optional[Tensor] = None, chain: bool = False) -> Tensor:
        """one view at one time, ``chunk`` (default RENDER_CHUNK) rays per render_rays call.  ``chain=True``: the frame as ONE launch
        chain, for the engines that have one (_render_image_chain)"""
        chunk = chunk or self.RENDER_CHUNK
        if chain:
            return self._render_image_chain(rays_o, rays_d, time, n_samples, chunk, bg)
        return render_chunks(lambda o, d: self.render_rays(o, d, time.reshape(1, 1).to(self.device), n_samples, bg=bg), rays_o, rays_d, chunk,
                             self.device)

    def _render_image_chain(self, rays_o: Tensor, rays_d: Tensor, time: Tensor, n_samples: int, chunk: int, bg: Optional[Tensor]) -> Tensor:
        raise NotImplementedError(f"render_image(chain=True): {type(self).__name__} has no evaluation launch chain (Part3InstantEngine "
                                  "renders through nerf_p3_render_rays_fwd)")


class GridEngine(DynamicEngine):
    """An engine that samples through an occupancy grid (``grid``: running density, ``binary_grid``: its threshold) of half-width
    ``grid_bound``, which the subclass sets."""

    def __init__(self, cfg: dict, device: str, seed: int, world_size: int):
        super().__init__(cfg, device, seed, world_size)
        res = int(cfg.get("grid_resolution", 128))
        self.grid_threshold = float(cfg.get("grid_threshold", 0.01))
        self.grid = torch.zeros(res, res, res, device=self.device)
        self.binary_grid = torch.ones(res, res, res, dtype=torch.bool, device=self.device)

    def prepare_batch(self, rays_o: Tensor, rays_d: Tensor, n_samples: int, first_ray: int = 0):
        """queues the compaction of one batch; (its handle, the jitter / noise counter of the batch)"""
        self._counter += 1
        return ops.sample_compact_async(rays_o, rays_d, self.near, self.far, n_samples, self.binary_grid, self.grid_bound,
                                        jitter=(self.seed, self._counter), first_ray=first_ray), self._counter

    def _lattice(self):
        """(the occupancy lattice's points [res^3,3], zero view directions for one batch of them)"""
        return ops.grid_lattice(self.grid_bound, self.grid.shape[0], self.device), torch.zeros(2 ** 18, 3, device=self.device)

    def lattice_density(self, lattice, t_val: float):
        """yields (i, sigma of the lattice points [i, i + 2^18)) at time ``t_val``; how the times combine is the engine's"""
        pts, zeros = lattice
        for i in range(0, pts.shape[0], zeros.shape[0]):
            p = pts[i:i + zeros.shape[0]]
            yield i, self.field(p, zeros[:p.shape[0]], torch.full((p.shape[0],), float(t_val), device=self.device))[1]

    @torch.no_grad()
    def render_rays(self, rays_o: Tensor, rays_d: Tensor, times: Tensor, n_samples: int, bg: Optional[Tensor] = None):
        """(rgb [R,3], depth [R], acc [R]) with per-ray times [R,1] (or one time), no jitter"""
        z, slots, pts, dirs = ops.sample_compact(rays_o, rays_d, self.near, self.far, n_samples, self.binary_grid, self.grid_bound)
        R = rays_o.shape[0]
        bg = self.bg if bg is None else bg
        if pts.shape[0] == 0:
            return bg.expand(R, 3).clone(), torch.zeros(R, device=self.device), torch.zeros(R, device=self.device)
        _, t_def = sample_inputs(slots, pts, times.expand(R, 1) if times.numel() == 1 else times, R, n_samples)
        rgb, sigma, _ = self.field(pts, dirs, t_def)
        return ops.composite_indexed(rgb, sigma, slots, z, rays_d, bg)
