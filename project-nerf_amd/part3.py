"""Part 3 (D-NeRF with an MLP deformation field) on a hash-grid canonical field -- ``canonical_type: instant`` -- as a
flat-parameter training engine on fused HIP chains: the loop body of reference run_part3 (run.py:1040-1222) with
NeuralField('part3') (src/core.py:79-146, 233-281).

    batch -> compaction -> t', x' (+ noise) -> deformation chain (csrc/p3deform.hip: Fourier codes of x', t' -> 128 -> 128
    -> 128 -> 3, x_c = x + dx) -> canonical hash encoding at x_c -> canonical chain (Part 4's, csrc/p4mlp.hip: the same
    InstantNeRFDecoder on [hash (32) | time code (21)]) -> compositing + MSE + displacement regulariser + backward (one
    kernel) -> canonical chain bwd + wgrad -> hash input gradient + counted scatter -> deformation chain bwd + wgrad
    -> [temporal / consistency probes through the same kernels] -> [all-reduce] -> TV on the canonical table + ONE
    global-norm clip + AdamW (one group, cosine schedule).

No torch autograd, torch.optim or library GEMM in the loop.  The canonical decoder lives at Part 4's offsets of a Part 4
parameter vector (its deformation slots stay zero and unused), so Part 4's kernels run unchanged through their existing
entry points; the deformation MLP follows it in the same flat vector.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib, ops
from . import part4 as p4
from .dynamic_engine import GridEngine, clip_adamw_flat, composite_mse_reg_bwd, normsq_flat, sample_inputs
from .flat_engine import grid_update_chain, render_counted_chain

Tensor = torch.Tensor
P = lambda t: None if t is None else t.data_ptr()

DEFORM0 = p4.N_PARAMS                                 # the deformation MLP follows the Part 4 vector
W1, B1, W2, B2, W3, B3, W4, B4, N_DEFORM = 0, 10752, 10880, 27264, 27392, 43776, 43904, 44288, 44291
N_PARAMS = DEFORM0 + N_DEFORM
TABLE_KEY = "canonical_repr.encoding.params"
# (state-dict key, offset into the flat network vector, shape)
MODULE_SLICES = (
    ("decoder.sigma_net.params", p4.S1, (64 * 64 + 16 * 64,)),
    ("decoder.color_net.params", p4.C1, (64 * 48 + 64 * 64 + 16 * 64,)),
    ("deform_net.net.0.weight", DEFORM0 + W1, (128, 84)), ("deform_net.net.0.bias", DEFORM0 + B1, (128,)),
    ("deform_net.net.2.weight", DEFORM0 + W2, (128, 128)), ("deform_net.net.2.bias", DEFORM0 + B2, (128,)),
    ("deform_net.net.4.weight", DEFORM0 + W3, (128, 128)), ("deform_net.net.4.bias", DEFORM0 + B3, (128,)),
    ("deform_net.net.6.weight", DEFORM0 + W4, (3, 128)), ("deform_net.net.6.bias", DEFORM0 + B4, (3,)),
)


def supported(cfg: dict) -> Optional[str]:
    """None if the fused chains are compiled for this configuration, else the reason they are not.  Table size, base
    resolution, level scale and bound are free."""
    if cfg.get("mode") != "part3":
        return f"mode={cfg.get('mode')} (compiled: part3)"
    if cfg.get("canonical_type", "nerf") != "instant":
        return f"canonical_type={cfg.get('canonical_type', 'nerf')} (compiled: instant)"
    if cfg.get("direct_time_conditioning", False):
        return "direct_time_conditioning=True (compiled: False)"
    want = {"L_embed": (10, 0), "L_embed_time": (10, 10), "L_embed_dir": (4, 4), "deform_hidden_dim": (128, 128),
            "deform_num_layers": (4, 4), "hidden_dim": (64, 64), "n_levels": (16, 16), "n_features_per_level": (2, 2)}
    for key, (compiled, default) in want.items():
        if cfg.get(key, default) != compiled:
            return f"{key}={cfg.get(key, default)} (compiled: {compiled})"
    if not cfg.get("use_positional_encoding", True):
        return "use_positional_encoding=False (compiled: True)"
    return None


def _check_count():
    n = _lib.load().nerf_p3_deform_param_count()
    if n != N_DEFORM:
        raise _lib.NerfHipError(f"libnerf_hip.so reports {n} Part 3 deformation parameters, this binding expects {N_DEFORM}")


# --------------------------------------------------------------------------------------------------- deformation chain
def deform_pack(params: Tensor, packed: Optional[Tensor] = None) -> Tensor:
    """fragment image of the deformation MLP ``params`` [44291] (deform_net.net.{0,2,4,6}.{weight,bias} concatenated)"""
    lib = _lib.load()
    _check_count()
    if params.numel() != N_DEFORM or not params.is_contiguous():
        raise ValueError(f"Part 3 deformation MLP: {N_DEFORM} contiguous parameters expected, got {params.numel()}")
    if packed is None:
        packed = torch.empty(lib.nerf_p3_deform_packed_bytes(), dtype=torch.uint8, device=params.device)
    _lib.check(lib.nerf_p3_deform_pack(P(params), P(packed), ops._stream()), "nerf_p3_deform_pack")
    return packed


def deform_workspace_bytes(n: int) -> int:
    return max(_lib.load().nerf_p3_deform_workspace_bytes(n), 256)


def deform_fwd(packed: Tensor, pts: Tensor, t: Tensor, x_code: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
    """(delta_x [n,3], x_c [n,3]) of the deformation MLP at the codes of ``x_code`` (default pts) and t [n]; x_c = pts + delta_x.
    ``workspace`` (>= deform_workspace_bytes(n) bytes): training forward, keeps what deform_bwd reads."""
    lib = _lib.load()
    pts = ops._dev(pts, "pts")
    t = ops._dev(t.reshape(-1), "t")
    n = pts.shape[0]
    dx, xc = torch.empty(n, 3, device=pts.device), torch.empty(n, 3, device=pts.device)
    if workspace is not None and workspace.numel() < deform_workspace_bytes(n):
        raise ValueError("deform_fwd: workspace too small")
    _lib.check(lib.nerf_p3_deform_fwd(P(packed), P(workspace), P(None if x_code is None else ops._dev(x_code, "x_code")), P(pts), P(t), n,
                                      P(dx), P(xc), 1 if workspace is not None else 0, ops._stream()), "nerf_p3_deform_fwd")
    return dx, xc


def deform_bwd(packed: Tensor, workspace: Tensor, d_dx: Tensor, grads: Tensor) -> None:
    """ADDS the weight and bias gradients of the last training deform_fwd on ``workspace`` into ``grads`` [44291]"""
    lib = _lib.load()
    d_dx = ops._dev(d_dx, "d_dx")
    if grads.numel() != N_DEFORM or not grads.is_contiguous():
        raise ValueError("deform_bwd: grads must be a contiguous [44291] tensor")
    _lib.check(lib.nerf_p3_deform_bwd(P(packed), P(workspace), P(d_dx), d_dx.shape[0], P(grads), ops._stream()), "nerf_p3_deform_bwd")


def probe_draws(cfg: dict, step: int, device, generator=None) -> Optional[Dict[str, Tensor]]:
    """The probe points dynamic.part3_regularisers draws on this step (the same keys, defaults, counts and draw order), or
    None on a step that evaluates neither term."""
    warm = cfg.get("grid_warmup_iters", 256)
    bound = float(cfg.get("scene_bound", 1.2))
    rand = lambda *shape: torch.rand(*shape, device=device, generator=generator)
    probes = {}
    if cfg.get("use_temporal_smooth", True) and step > warm and step % 2 == 0:
        eps, n = float(cfg.get("temporal_epsilon", 0.02)), int(cfg.get("temporal_n_samples", 256))
        probes["temporal_x"] = (rand(n, 3) * 2 - 1) * bound
        probes["temporal_t"] = rand(n, 1) * (1.0 - eps)
    if cfg.get("use_unsupervised_consistency", False) and step > warm and step % 4 == 0:
        n = min(int(cfg.get("unsup_n_samples", 512)), 512)
        probes["unsup_t"] = rand(n, 1)
        probes["unsup_x"] = (rand(n, 3) * 2 - 1) * bound
    return probes or None


def deform_probe_regularisers(cfg: dict, packed_d: Tensor, workspace, g_deform: Tensor, probes: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """temporal smoothness and unsupervised consistency of dynamic.part3_regularisers on the given probes: deformation
    chain forward (one batch of rows), the terms and their gradients w.r.t. delta_x as elementwise arithmetic, deformation
    chain backward ADDING into g_deform [N_DEFORM].  ``workspace(n)``: a deformation workspace for n rows.  Returns the weighted
    terms.  Shared by the Part 3 engines."""
    rows_x, rows_t, spans, terms = [], [], {}, {}
    if "temporal_x" in probes:
        eps = float(cfg.get("temporal_epsilon", 0.02))
        x, t = probes["temporal_x"], probes["temporal_t"].reshape(-1)
        m = x.shape[0]
        spans["tmp"] = (0, m)
        rows_x += [x, x]
        rows_t += [t, t + eps]
    if "unsup_x" in probes:
        at = sum(r.shape[0] for r in rows_x)
        spans["unsup"] = (at, probes["unsup_x"].shape[0])
        rows_x.append(probes["unsup_x"])
        rows_t.append(probes["unsup_t"].reshape(-1))
    if not rows_x:
        return terms
    X, T = torch.cat(rows_x).contiguous(), torch.cat(rows_t).contiguous()
    ws = workspace(X.shape[0])
    dx, _ = deform_fwd(packed_d, X, T, workspace=ws)
    g = torch.zeros_like(dx)
    if "tmp" in spans:
        lo, m = spans["tmp"]
        w = float(cfg.get("temporal_smooth_weight", 1e-4)) * 2
        diff = dx[lo:lo + m] - dx[lo + m:lo + 2 * m]
        terms["temporal"] = torch.mean(diff ** 2) * w
        g[lo:lo + m] += 2 * w * diff / diff.numel()
        g[lo + m:lo + 2 * m] -= 2 * w * diff / diff.numel()
    if "unsup" in spans:
        lo, m = spans["unsup"]
        w = float(cfg.get("unsup_consistency_weight", 0.001)) * 4
        mean = dx[lo:lo + m].mean(dim=0, keepdim=True)
        terms["unsup"] = torch.mean(torch.abs(mean)) * w
        g[lo:lo + m] += (w / 3.0) * torch.sign(mean).expand(m, 3) / m
    deform_bwd(packed_d, ws, g, g_deform)
    return terms


# --------------------------------------------------------------------------------------------------- engine
class Part3InstantEngine(GridEngine):
    """Flat-parameter training / rendering engine of mode part3 with canonical_type instant (module docstring)."""
    SLACK = (1.25, 256)

    def __init__(self, cfg: dict, device: str = "cuda", seed: int = 0, world_size: int = 1):
        why = supported(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Part 3 chains are not compiled for {why}")
        _check_count()
        p4._check_count()
        super().__init__(cfg, device, seed, world_size)
        self.bound = float(cfg.get("scene_bound", 1.0))                 # the canonical grid's bound (src/core.py:118)
        self.grid_bound = float(cfg.get("grid_bound", cfg.get("scene_bound", 1.5)))
        self.levels = ops.HashLevelTable(cfg.get("n_levels", 16), cfg.get("log2_hashmap_size", 19), cfg.get("base_resolution", 16),
                                         cfg.get("per_level_scale", 1.5))
        n_tab = self.levels.entries * 2
        g = torch.Generator().manual_seed(seed)
        self.table = ((torch.rand(n_tab, generator=g) * 2 - 1) * 1e-4).to(self.device)
        self.table_h = torch.empty(n_tab, dtype=torch.float16, device=self.device)
        self.g_table = torch.zeros(n_tab, device=self.device)
        self.net = torch.zeros(N_PARAMS, device=self.device)
        self._g_net_scalars = torch.zeros(N_PARAMS + 4, device=self.device)
        self.g_net = self._g_net_scalars[:N_PARAMS]
        self.state = {"table": (torch.zeros_like(self.table), torch.zeros_like(self.table)),
                      "net": (torch.zeros_like(self.net), torch.zeros_like(self.net))}
        self.packed_c = torch.empty(_lib.load().nerf_p4_packed_bytes(), dtype=torch.uint8, device=self.device)
        self.packed_d = torch.empty(_lib.load().nerf_p3_deform_packed_bytes(), dtype=torch.uint8, device=self.device)
        self.tv = float(cfg.get("tv_loss_weight", 1e-6)) if cfg.get("use_tv_loss", True) else 0.0
        # two-bit signs of the TV term; zeroed once (a one-table call never reads a byte pass 1 left unwritten)
        self._tv_codes = torch.zeros((n_tab + 3) // 4, dtype=torch.uint8, device=self.device)
        self.repack()

    # -- parameters ------------------------------------------------------------------------------------------
    @property
    def deform_params(self) -> Tensor:
        return self.net[DEFORM0:]

    @property
    def g_deform(self) -> Tensor:
        return self.g_net[DEFORM0:]

    def _pack_nets(self) -> None:
        p4.pack(self.net[:p4.N_PARAMS], self.packed_c)
        deform_pack(self.deform_params, self.packed_d)

    def repack(self) -> None:
        self._pack_nets()
        ops.f32_to_f16(self.table, self.table_h)

    @staticmethod
    def slice_table():
        """(key, 'net' or 'table', offset, shape) of every module parameter inside the engine's flat buffers"""
        return [(k, "net", off, shape) for k, off, shape in MODULE_SLICES] + [(TABLE_KEY, "table", 0, None)]

    def load_from_model(self, model) -> None:
        with torch.no_grad():
            self.net.zero_()                       # Part 4's deformation slots: zero and unused
        super().load_from_model(model)

    def _p4_ws(self, n: int, which: str = "batch") -> p4.Workspace:
        return p4.Workspace(n, self.device, buf=self._buf("p4_" + which, p4.Workspace.bytes(n)))

    def _deform_ws(self, n: int, which: str = "batch") -> Tensor:
        return self._buf("p3_" + which, deform_workspace_bytes(n))

    def _hash_scratch(self, n: int) -> Tensor:
        return self._buf("hash", ops.hash_encode_bwd_workspace_bytes(n, self.levels.n_levels))

    # -- field -----------------------------------------------------------------------------------------------
    def _canonical(self, xc: Tensor, t: Tensor, dirs: Tensor, ws: p4.Workspace, train: bool):
        lib = _lib.load()
        n = xc.shape[0]
        ops.hash_encode_fwd_nat(xc, self.table_h.view(-1, 2), self.levels, self.bound, ws.nat(3), fp16=True)
        rgb, sigma = torch.empty(n, 3, device=self.device), torch.empty(n, device=self.device)
        _lib.check(lib.nerf_p4_canon_fwd(P(self.packed_c), P(ws.buf), P(t), P(dirs), n, P(rgb), P(sigma), 1 if train else 0, ops._stream()),
                   "nerf_p4_canon_fwd")
        return rgb, sigma

    @torch.no_grad()
    def field(self, pts: Tensor, dirs: Tensor, t: Tensor):
        """(rgb [n,3], sigma [n], delta_x [n,3]) at points with per-point times, evaluation mode (no noise)"""
        pts, dirs, t = pts.contiguous(), dirs.contiguous(), t.reshape(-1).contiguous()
        n = pts.shape[0]
        if n == 0:
            return pts.new_zeros(0, 3), pts.new_zeros(0), pts.new_zeros(0, 3)
        dx, xc = deform_fwd(self.packed_d, pts, t)
        rgb, sigma = self._canonical(xc, t, dirs, self._p4_ws(n, "eval"), False)
        return rgb, sigma, dx

    _chain_ws = None           # render_image(chain=True): one workspace per (chunk, n_samples)
    _chain_time = None         # ... and the one time word its kernels read

    def _render_image_chain(self, rays_o: Tensor, rays_d: Tensor, time: Tensor, n_samples: int, chunk: int, bg: Optional[Tensor]) -> Tensor:
        """the frame as ONE launch chain (nerf_p3_render_rays_fwd): the chunks' active counts and the time stay on the device, no host
        read, no time vector, no delta_x and no allocation per chunk; the same bits as the loop"""
        if self._chain_ws is None:
            self._chain_ws, self._chain_time = {}, torch.zeros(1, device=self.device)
        self._chain_time.copy_(time.reshape(1))
        bg = self.bg if bg is None else bg
        return render_counted_chain(
            lambda o, d, chunk, ws: ops.p3_render_rays_fwd(self.packed_d, self.packed_c, self.table_h.view(-1, 2), self.levels, self.bound,
                                                           self.binary_grid, self.grid_bound, o, d, n_samples, self.near, self.far,
                                                           self._chain_time, bg, chunk, workspace=ws),
            ops.p3_render_workspace_bytes, self._chain_ws, rays_o, rays_d, n_samples, chunk, self.device)

    def compute_gradients(self, rays_o: Tensor, rays_d: Tensor, target: Tensor, times: Tensor, n_samples: int, prepared=None,
                          first_ray: int = 0, bg: Optional[Tensor] = None, sync_grads_async=None, probes=None) -> Tensor:
        """Forward + backward of one batch: fills g_net / g_table with the gradient of MSE + deformation_reg_weight *
        mean(mean_delta_x^2) (+ the probe terms) of the LOCAL rays and returns the RGB loss.  ``sync_grads_async(view)``:
        data-parallel hook (a summing all-reduce; apply_gradients divides by the world size)."""
        lib = _lib.load()
        R = rays_o.shape[0]
        prepared, counter = prepared if prepared is not None else self.prepare_batch(rays_o, rays_d, n_samples, first_ray)
        z, slots, pts, dirs = prepared.get()
        n = pts.shape[0]
        bg = self.bg if bg is None else bg
        self._g_net_scalars.zero_()
        scalars = self._g_net_scalars[N_PARAMS:]
        loss, reg = scalars[0:1], scalars[1:2]
        if n == 0:
            self.g_table.zero_()
            loss = ((bg.expand(R, 3) - target) ** 2).mean().reshape(1)
        else:
            x_def, t_def = sample_inputs(slots, pts, times, R, n_samples, self.std_x, self.std_t, self.seed, counter, first_ray)
            dws = self._deform_ws(n)
            dx, xc = deform_fwd(self.packed_d, pts, t_def, x_code=x_def, workspace=dws)
            ws = self._p4_ws(n)
            rgb, sigma = self._canonical(xc, t_def, dirs, ws, True)
            d_rgb, d_sigma, d_dx = composite_mse_reg_bwd(rgb, sigma, slots, z, rays_d, bg, target, dx, self.reg_weight, R, n_samples, loss, reg,
                                                         ops.sum_ws(self.device))
            _lib.check(lib.nerf_p4_canon_bwd(P(self.packed_c), P(ws.buf), P(rgb), P(sigma), P(d_rgb), P(d_sigma), n, P(self.g_net), None, None,
                                             ops._stream()), "nerf_p4_canon_bwd")
            d_feat = ws.d_feat(3)
            # d x_c through the grid ADDED to the regulariser's d delta_x (x_c = x + delta_x), then the counted scatter
            ops.hash_encode_bwd_input(xc, self.table_h.view(-1, 2), self.levels, self.bound, d_feat, add_to=d_dx)
            ops.hash_encode_bwd(xc, self.levels, self.bound, d_feat, self.g_table, workspace=self._hash_scratch(n), overwrite=True)
            deform_bwd(self.packed_d, dws, d_dx, self.g_deform)
        self.last_reg = reg[0]
        self.last_terms = self._probe_regularisers(probes) if probes else {}
        self._sync_grads(sync_grads_async, self.g_table, self.g_net)
        return loss[0]

    def _probe_regularisers(self, probes: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """temporal smoothness and unsupervised consistency on the given probes (deform_probe_regularisers), ADDING into g_net"""
        return deform_probe_regularisers(self.cfg, self.packed_d, lambda n: self._deform_ws(n, "probes"), self.g_deform, probes)

    def apply_gradients(self) -> None:
        """TV-L1 on the canonical table, ONE global-norm clip over every parameter (clip_grad_norm_(model.parameters()),
        run.py:1174) and AdamW as one group with the cosine schedule; after a summing all-reduce the data gradient is
        averaged (1/world), the TV term is added unscaled."""
        scale = 1.0 / self.world_size
        normsq = self._normsq_ws
        n_tab = self.table.numel()
        codes = self._tv_codes if self.tv != 0.0 else None
        # pass 1: the table STORES the squared norm (no zeroing launch), the networks add to it
        ops.tv_normsq_codes(self.table, self.g_table, n_tab, normsq, tv_weight=self.tv, grad_scale=scale, codes=codes)
        normsq_flat(self.net, self.g_net, N_PARAMS, scale, normsq, first=False)
        lr = self.lr()                             # the rate of THIS step: scheduler.step() follows optimizer.step()
        self.step_count += 1
        # pass 2: the whole table is the "lo" range of ONE table (tv_split = n): the seam path of two ranges is never reached
        ops.adamw_clip_step_tv(self.table, self.g_table, *self.state["table"], n_tab, self.step_count, lr, normsq, weight_decay=self.wd,
                               max_norm=self.max_norm, grad_scale=scale, codes=codes, tv=(self.tv, n_tab), shadow_f16=self.table_h)
        clip_adamw_flat(self.net, self.g_net, self.state["net"], N_PARAMS, self.step_count, lr, self.wd, normsq, self.max_norm, scale)
        self._pack_nets()

    # -- occupancy grid --------------------------------------------------------------------------------------
    @torch.no_grad()
    def update_grid(self, times, chain: bool = False) -> float:
        """Part 3's DensityGrid refresh (reference run.py:1191-1222, renderer.py:87-101): density on the lattice at each of
        ``times``, running maximum with decay 1.0 -- the union over the times."""
        if chain:
            raise NotImplementedError("update_grid(chain=True): this keyword names the Part 4 dual-hash field's refresh chain "
                                      "(nerf_p4_grid_update); Part 3's density-only chain is update_grid_chain(times)")
        res = self.grid.shape[0]
        lattice = self._lattice()
        ratio = 0.0
        for t_val in times:
            sig = torch.empty(res ** 3, device=self.device)
            for i, s in self.lattice_density(lattice, t_val):
                sig[i:i + s.shape[0]] = s
            self.binary_grid, ratio = ops.grid_threshold(sig.view(res, res, res), self.grid_threshold, prev=self.grid, decay=1.0)
        return ratio

    _GRID_SLAB = 2 ** 18       # cells per slab of the chain refresh: the loop form's batch
    _grid_ws = None            # update_grid_chain: one slab's x_c and canonical operand image

    @torch.no_grad()
    def update_grid_chain(self, times) -> float:
        """update_grid(times) as ONE density-only launch chain (nerf_p3_grid_update): no lattice tensor, no time vectors, no
        delta_x, no colour-net, one sync instead of one per time, one workspace kept on the engine; the same bits as the loop.
        ``self.grid`` is updated in place and ``binary_grid`` is a new tensor, as the loop leaves them."""
        return grid_update_chain(                        # its one host sync; the grid it installs is ``self.grid`` itself
            self, lambda slab, ws: ops.p3_grid_update(self.packed_d, self.packed_c, self.table_h.view(-1, 2), self.levels, self.bound, times,
                                                      self.grid.shape[0], self.grid_bound, self.grid_threshold, self.grid, decay=1.0,
                                                      slab_cells=slab, workspace=ws),
            ops.p3_grid_update_workspace_bytes)
