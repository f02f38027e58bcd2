"""Part 4 dual-hash dynamic field on the fused HIP chains (csrc/p4mlp.hip): the operator behind
``NeuralField('part4').forward`` (reference src/core.py:282-352) and the flat-parameter training engine of the loop
body of reference run_part4 (run.py:1808-1990).

Two entry points over the same kernels:
  * ``field(...)``: differentiable operator for the module path (NeuralField + torch.optim): the parameters stay the
    module's own nn.Parameters (reference state-dict keys), autograd receives their gradients from the HIP backward;
  * ``DualHashEngine``: owns flat parameter / gradient / Adam vectors and issues the whole step -- compaction, the four
    hash encodings, the two fused MLP chains, compositing + MSE + displacement regulariser + their backward, the hash
    scatters, TV terms, ONE global-norm clip and AdamW with the reference's per-group learning rates -- with no torch
    autograd, no torch.optim and no library GEMM in the loop.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib, ops
from .dynamic_engine import GridEngine, clip_adamw_flat, composite_mse_reg_bwd, normsq_flat, sample_inputs, wait_all
from .flat_engine import ViewSlots, grid_update_chain

Tensor = torch.Tensor
P = lambda t: None if t is None else t.data_ptr()

# offsets into the flat parameter vector (csrc/p4mlp.hip)
T1W, T1B, T2W, T2B, D1, D2, D3, S1, S2, C1, C2, C3, SCALE, N_PARAMS = (0, 1344, 1408, 5504, 5568, 11712, 15808, 16832, 20928, 21952,
                                                                          25024, 29120, 30144, 30145)
# (state-dict key, offset, element count) of the module parameters inside the flat vector
MODULE_SLICES = (
    ("time_modulation.net.0.weight", T1W, 64 * 21), ("time_modulation.net.0.bias", T1B, 64),
    ("time_modulation.net.2.weight", T2W, 64 * 64), ("time_modulation.net.2.bias", T2B, 64),
    ("deform_decoder.deform_net.params", D1, 64 * 96 + 64 * 64 + 16 * 64),
    ("decoder.sigma_net.params", S1, 64 * 64 + 16 * 64), ("decoder.color_net.params", C1, 64 * 48 + 64 * 64 + 16 * 64),
    ("deform_decoder.displacement_scale", SCALE, 1),
)
GRIDS = ("deform_grid_start", "deform_grid_mid", "deform_grid_end", "canonical_repr")


def supported(cfg: dict) -> Optional[str]:
    """None if the fused chains are compiled for this configuration, else the reason they are not."""
    want = {"L_embed_time": (10, 10), "L_embed_dir": (4, 4), "time_modulation_dim": (64, 64), "time_modulation_layers": (2, 2),
            "deform_hidden_dim": (64, 64), "hidden_dim": (64, 64), "deform_n_levels": (12, 14), "n_levels": (16, 16),
            "deform_n_features_per_level": (2, 2), "n_features_per_level": (2, 2)}
    for key, (compiled, default) in want.items():
        if cfg.get(key, default) != compiled:
            return f"{key}={cfg.get(key, default)} (compiled: {compiled})"
    return None


def _check_count():
    n = _lib.load().nerf_p4_param_count()
    if n != N_PARAMS:
        raise _lib.NerfHipError(f"libnerf_hip.so reports {n} Part 4 parameters, this binding expects {N_PARAMS}")


class Workspace:
    """hash operand images, every training image, the d-feature arrays of ``n`` points (the kernels derive the layout from n);
    ``buf``: a caller-owned buffer of at least ``Workspace.bytes(n)`` bytes to lay it out in (the engine's grow-only buffer).
    ``train=False``: evaluation only -- the four operand images, which lead the layout (nerf_p4_infer_workspace_bytes: 256 bytes
    per point instead of ~2.9 KB); the forward chains touch nothing else when they do not stash."""

    @staticmethod
    def bytes(n: int, train: bool = True) -> int:
        lib = _lib.load()
        return max(lib.nerf_p4_workspace_bytes(n) if train else lib.nerf_p4_infer_workspace_bytes(n), 256)

    def __init__(self, n: int, device, buf: Optional[Tensor] = None, train: bool = True):
        lib = _lib.load()
        self.n, self.train = n, train
        need = Workspace.bytes(n, train)
        if buf is not None and buf.numel() < need:
            raise ValueError(f"Part 4 workspace: {need} bytes needed for {n} points, {buf.numel()} given")
        self.buf = buf if buf is not None else torch.empty(need, dtype=torch.uint8, device=device)
        self._off = [lib.nerf_p4_workspace_offset(n, k) for k in range(8)]

    def nat(self, k: int) -> Tensor:                     # 0..2 deformation grids, 3 canonical
        return self.buf[self._off[k]:]

    def d_feat(self, k: int) -> Tensor:                  # 0..2 [n,24], 3 [n,32]
        width = 32 if k == 3 else 24
        if not self.train:
            raise ValueError("Part 4 workspace: an evaluation workspace holds no d features")
        return self.buf[self._off[4 + k]:self._off[4 + k] + self.n * width * 4].view(torch.float32).view(self.n, width)


def pack(params: Tensor, packed: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    _check_count()
    params = ops._dev(params, "params")
    if params.numel() != N_PARAMS:
        raise ValueError(f"Part 4 networks: {N_PARAMS} parameters expected, got {params.numel()}")
    if packed is None:
        packed = torch.empty(lib.nerf_p4_packed_bytes(), dtype=torch.uint8, device=params.device)
    _lib.check(lib.nerf_p4_pack(P(params), P(packed), ops._stream()), "nerf_p4_pack")
    return packed


def forward_chain(packed, params, tables, levels_d, levels_c, bound, pts, x_def, t_def, dirs, ws: Workspace, train: bool,
                  blend: Optional[Tensor] = None):
    """hash encodings + both fused chains -> (rgb [n,3], sigma [n], delta_x [n,3], x_canonical [n,3]).
    ``tables``: [start, mid, end, canonical], each fp32 [E,2] or an fp16 copy."""
    lib = _lib.load()
    n = pts.shape[0]
    dev = pts.device
    if train and not ws.train:
        raise ValueError("Part 4 forward: the training chains stash into the full workspace (Workspace(n, train=True))")
    x_in = pts if x_def is None else x_def
    # the engine's three deformation tables are views of one flat fp16 buffer: one launch; separate tensors: one launch each
    if not ops.hash_encode_fwd_nat_tables(x_in, tables[:3], levels_d, bound, [ws.nat(k) for k in range(3)], fp16=True):
        for k in range(3):
            ops.hash_encode_fwd_nat(x_in, tables[k], levels_d, bound, ws.nat(k), fp16=True)
    dx, xc = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    _lib.check(lib.nerf_p4_deform_fwd(P(packed), P(params), P(ws.buf), P(pts), P(t_def), P(blend), n, P(dx), P(xc), 1 if train else 0,
                                      ops._stream()), "nerf_p4_deform_fwd")
    if dirs is None:
        return None, None, dx, xc
    ops.hash_encode_fwd_nat(xc, tables[3], levels_c, bound, ws.nat(3), fp16=True)
    rgb, sigma = torch.empty(n, 3, device=dev), torch.empty(n, device=dev)
    _lib.check(lib.nerf_p4_canon_fwd(P(packed), P(ws.buf), P(t_def), P(dirs), n, P(rgb), P(sigma), 1 if train else 0, ops._stream()),
               "nerf_p4_canon_fwd")
    return rgb, sigma, dx, xc


def backward_chain(packed, params, table_c, levels_d, levels_c, bound, x_in, xc, ws: Workspace, rgb, sigma, d_rgb, d_sigma,
                   d_dx_extra, g_net, g_tables, hash_ws=None, after_canonical=None, after_grid=None, overwrite=False, tables_ws=None,
                   extra_in_place=False, spec=None):
    """Adds the gradients of one batch into ``g_net`` [30145] and ``g_tables`` (4 tensors [E*2]); ``overwrite`` (needs
    ``hash_ws``): the table gradients are STORED instead (no zeroing by the caller, no read-back -- the engine's data batch);
    ``tables_ws(n, n_levels, n_tables)``: workspace for scattering to the three deformation grids in one pass.  ``d_dx_extra`` [n,3] or
    None: gradient reaching delta_x directly (displacement regulariser, a caller's loss on delta_x); rgb None: the
    deformation chain alone (regulariser probes).  ``after_*`` callbacks: data-parallel hooks (ranges that are final).
    ``extra_in_place`` (fp16 canonical table): d_dx_extra is the caller's scratch -- the gradient through x_canonical is added INTO it
    (no zeroing launch, no separate add).  ``spec`` = (SpeculativeScatter of the canonical grid's workspace, of the deformation grids',
    occupancy-grid identity): the engine's steady state -- both scatters skip their count passes when the estimates hold."""
    lib = _lib.load()
    n = x_in.shape[0]
    d_dx = d_dx_extra
    # the engine's steady state: the scatters skip their count passes (specbwd.py) -- capacities from the last call's true counts
    spec_c = spec_d = None
    use_c = use_d = False
    hws_c = hws_d = None
    if spec is not None and overwrite and tables_ws is not None and hash_ws is not None and rgb is not None:
        spec_c, spec_d, grid_id = spec
        hws_c, hws_d = hash_ws(n, levels_c.n_levels), tables_ws(n, levels_d.n_levels, 3)
        use_c = table_c.dtype == torch.float16 and spec_c.ok(hws_c.data_ptr(), grid_id, n)
        use_d = spec_d.ok(hws_d.data_ptr(), grid_id, n)
    if rgb is not None:
        amax_c = lm_c = None
        if use_c:                                # the chain hands its d features over level-major, inside the scatter's workspace
            spec_c.begin(hws_c)
            amax_c, lm_c = ops.hash_bwd_slots(hws_c, n, levels_c.n_levels)
        _lib.check(lib.nerf_p4_canon_bwd(P(packed), P(ws.buf), P(rgb), P(sigma), P(d_rgb), P(d_sigma), n, P(g_net), amax_c, lm_c, ops._stream()),
                   "nerf_p4_canon_bwd")
        d_feat_c = ws.d_feat(3)
        in_place = extra_in_place and d_dx_extra is not None and table_c.dtype == torch.float16 and d_dx_extra.is_contiguous()
        d_xc = ops.hash_encode_bwd_input(xc, table_c.view(-1, 2), levels_c, bound, None if use_c else d_feat_c,
                                         add_to=d_dx_extra if in_place else None, grad_lm=lm_c)
        if use_c:
            status = spec_c.status_block()
            _lib.check(lib.nerf_hash_encode_bwd_ws_store_spec(P(xc), n, levels_c.n_levels, *levels_c.host_args(), float(bound), None,
                                                              P(g_tables[3]), P(hws_c), hws_c.numel(), status.data_ptr(), ops._stream()),
                       "nerf_hash_encode_bwd_ws_store_spec")
            spec_c.issued(hws_c, grid_id, n, status)
        else:
            ops.hash_encode_bwd(xc, levels_c, bound, d_feat_c, g_tables[3], workspace=hash_ws(n, levels_c.n_levels) if hash_ws else None,
                                overwrite=overwrite)
            if spec_c is not None:
                spec_c.counted(hws_c, grid_id, n)
        if after_grid is not None:
            after_grid(3)
        d_dx = d_xc if (d_dx_extra is None or in_place) else d_xc.add_(d_dx_extra)
    amax_d = lm_d = None
    if use_d:
        spec_d.begin(hws_d)
        amax_d, lm_d = ops.hash_bwd_slots(hws_d, n, 3 * levels_d.n_levels)
    _lib.check(lib.nerf_p4_deform_bwd(P(packed), P(params), P(ws.buf), P(d_dx.contiguous()), n, P(g_net), amax_d, lm_d, ops._stream()),
               "nerf_p4_deform_bwd")
    if after_canonical is not None:
        after_canonical()
    # the engine's overwrite form: the three deformation grids (views of one flat gradient buffer) in one pass of launches
    status = spec_d.status_block() if use_d else None
    if overwrite and tables_ws is not None and ops.hash_encode_bwd_tables(x_in, levels_d, bound, [ws.d_feat(k) for k in range(3)], g_tables[:3],
                                                                          tables_ws, spec_status=status, spec_lm=use_d):
        if use_d:
            spec_d.issued(hws_d, grid_id, n, status)
        elif spec_d is not None:
            spec_d.counted(hws_d, grid_id, n)
        if after_grid is not None:
            for k in range(3):
                after_grid(k)
        return
    if use_d:         # (cannot happen: the estimates come from a call that took the one-pass form on the same buffers)
        raise RuntimeError("Part 4 backward: the deformation grids' gradients were handed over level-major but their one-pass scatter is unavailable")
    for k in range(3):
        ops.hash_encode_bwd(x_in, levels_d, bound, ws.d_feat(k), g_tables[k], workspace=hash_ws(n, levels_d.n_levels) if hash_ws else None,
                            overwrite=overwrite)
        if after_grid is not None:
            after_grid(k)
    if spec_c is not None:                       # the per-grid calls went through the canonical grid's workspace
        spec_c.invalidate()


# --------------------------------------------------------------------------------------------------- module path
def flat_from_modules(model) -> Tensor:
    """the flat parameter vector of the fused chains, assembled (differentiably) from the module's own parameters"""
    sd = dict(model.named_parameters())
    return torch.cat([sd[key].reshape(-1) for key, _, _ in MODULE_SLICES])


class _Part4Field(torch.autograd.Function):
    """NeuralField('part4').forward on the fused chains; gradients w.r.t. the flat network parameters and the four
    hash tables (incl. the deformation grids, reached through d features / d x_canonical)."""

    @staticmethod
    def forward(ctx, flat, t0, t1, t2, tc, pts, x_def, t_def, dirs, levels_d, levels_c, bound, train):
        packed = pack(flat.detach())
        ws = Workspace(pts.shape[0], pts.device, train=train)       # evaluation: the operand images alone
        tables = [t.detach().view(-1, 2) for t in (t0, t1, t2, tc)]
        rgb, sigma, dx, xc = forward_chain(packed, flat.detach(), tables, levels_d, levels_c, bound, pts, x_def, t_def, dirs, ws, train)
        if train:
            ctx.save_for_backward(flat, tc, pts if x_def is None else x_def, xc, rgb, sigma)
            ctx.packed, ctx.ws, ctx.meta = packed, ws, (levels_d, levels_c, bound, [t.numel() for t in (t0, t1, t2, tc)])
        return rgb, sigma, dx

    @staticmethod
    def backward(ctx, d_rgb, d_sigma, d_dx):
        flat, tc, x_in, xc, rgb, sigma = ctx.saved_tensors
        levels_d, levels_c, bound, sizes = ctx.meta
        g_net = torch.zeros(N_PARAMS, device=flat.device)
        g_tables = [torch.zeros(s, device=flat.device) for s in sizes]
        scratch = lambda n, L: ops._hash_bwd_scratch(x_in, levels_c if L == levels_c.n_levels else levels_d)
        backward_chain(ctx.packed, flat.detach(), tc.detach(), levels_d, levels_c, bound, x_in, xc, ctx.ws, rgb, sigma,
                       d_rgb.contiguous(), d_sigma.contiguous(), d_dx.contiguous(), g_net, g_tables, hash_ws=scratch)
        return (g_net, g_tables[0], g_tables[1], g_tables[2], g_tables[3]) + (None,) * 8


def field(model, x: Tensor, d: Tensor, t: Tensor, x_deform: Optional[Tensor] = None):
    """(rgb [n,3], sigma [n,1], delta_x [n,3]) of NeuralField('part4') for positions x, unit view directions d and per-sample
    times t [n,1] (already noised by the caller if it wants noise); ``x_deform``: the (noised) positions the deformation
    grids are queried at (default x)."""
    x, d = ops._dev(x, "x"), ops._dev(d, "d")
    t_def = ops._dev(t.reshape(-1), "t")
    if x.shape[0] == 0:
        return x.new_zeros(0, 3), x.new_zeros(0, 1), x.new_zeros(0, 3)
    grids = [getattr(model, g) for g in GRIDS]
    train = torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())
    rgb, sigma, dx = _Part4Field.apply(flat_from_modules(model), *[g.encoding.params for g in grids], x,
                                       None if x_deform is None else ops._dev(x_deform, "x_deform"), t_def, d,
                                       grids[0].levels, grids[3].levels, float(grids[3].bound), train)
    return rgb, sigma.unsqueeze(-1), dx


# --------------------------------------------------------------------------------------------------- engine
class DualHashEngine(GridEngine):
    """Flat-parameter training / rendering engine of mode part4 (loop body of reference run_part4, run.py:1808-1990):

        batch -> compaction -> t', x' (+ noise) -> 3 deformation hash encodings -> deformation chain -> canonical hash
        encoding -> canonical chain -> compositing + MSE + displacement regulariser + backward (one kernel)
        -> canonical chain bwd + wgrad -> hash input gradient + scatter -> deformation chain bwd + wgrad -> 3 scatters
        -> [regulariser probes through the same kernels] -> [all-reduce] -> TV terms + ONE global-norm clip + AdamW
        (2x lr for the four grids, 5x for displacement_scale, cosine schedule) -> repack.
    """
    REG_WEIGHT = 0.01

    def __init__(self, cfg: dict, device: str = "cuda", seed: int = 0, world_size: int = 1):
        why = supported(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Part 4 chains are not compiled for {why}")
        _check_count()
        super().__init__(cfg, device, seed, world_size)
        self.bound = self.grid_bound = float(cfg.get("scene_bound", 1.5))      # the hash grids' and the occupancy grid's
        self.levels_d = ops.HashLevelTable(cfg.get("deform_n_levels", 14), cfg.get("deform_log2_hashmap_size", 19),
                                           cfg.get("deform_base_resolution", 16), cfg.get("deform_per_level_scale", 1.5))
        self.levels_c = ops.HashLevelTable(cfg.get("n_levels", 16), cfg.get("log2_hashmap_size", 19), cfg.get("base_resolution", 16),
                                           cfg.get("per_level_scale", 1.5))
        nd, nc = self.levels_d.entries * 2, self.levels_c.entries * 2
        self.table_sizes = [nd, nd, nd, nc]
        self.table_offsets = [0, nd, 2 * nd, 3 * nd]
        total = 3 * nd + nc
        g = torch.Generator().manual_seed(seed)
        # ONE flat buffer for the four grids (start | mid | end | canonical): one memset, one AdamW launch.  The buffers are allocated
        # padded to world equal slices of whole 1024-element blocks (the sharded optimiser's reduce-scatter / all-gather); the views
        # below are the tables themselves
        from .sharded import padded_length
        n_pad = padded_length(total, max(self.world_size, 1))
        self._tables_buf = torch.zeros(n_pad, device=self.device)
        self._tables_buf[:total] = ((torch.rand(total, generator=g) * 2 - 1) * 1e-4).to(self.device)
        self._tables_h_buf = torch.zeros(n_pad, dtype=torch.float16, device=self.device)
        self._g_tables_buf = torch.zeros(n_pad, device=self.device)
        self.tables, self.tables_h, self.g_tables = self._tables_buf[:total], self._tables_h_buf[:total], self._g_tables_buf[:total]
        self.shard = None                         # ShardedTableOptimizer once enable_sharded_optimizer() was called
        self.net = torch.zeros(N_PARAMS, device=self.device)
        # network gradients and the step's four scalars (loss, regulariser, squared gradient norm, spare) in one buffer: one fill per step
        self._g_net_scalars = torch.zeros(N_PARAMS + 4, device=self.device)
        self.g_net = self._g_net_scalars[:N_PARAMS]
        self._m_buf, self._v_buf = torch.zeros(n_pad, device=self.device), torch.zeros(n_pad, device=self.device)
        self.state = {"tables": (self._m_buf[:total], self._v_buf[:total]), "net": (torch.zeros_like(self.net), torch.zeros_like(self.net))}
        self.packed = torch.empty(_lib.load().nerf_p4_packed_bytes(), dtype=torch.uint8, device=self.device)
        self.tv_disp = float(cfg.get("tv_displacement_weight", 0.001)) / 3.0 if cfg.get("use_tv_displacement", True) else 0.0
        self.tv_canon = float(cfg.get("tv_loss_weight", 1e-5))
        self._scalars = self._g_net_scalars[N_PARAMS:]
        self._loss_ring = ViewSlots(torch.zeros(32768, 2, device=self.device))
        assert (3 * nd) % 4 == 0
        self._tv_codes = torch.empty((total + 3) // 4, dtype=torch.uint8, device=self.device)   # two-bit signs of the TV terms
        from .specbwd import SpeculativeScatter
        on = bool(cfg.get("speculative_hash_backward", True)) and not os.environ.get("NERF_NO_SPECULATIVE_BWD")      # env: A/B aid
        self.spec_c, self.spec_d = SpeculativeScatter(on), SpeculativeScatter(on)
        self._grid_ws = None           # update_grid(chain=True): one slab's two operand images and x_c
        self.repack()

    # -- parameters ------------------------------------------------------------------------------------------
    def table(self, k: int, half: bool = False) -> Tensor:
        src = self.tables_h if half else self.tables
        return src[self.table_offsets[k]:self.table_offsets[k] + self.table_sizes[k]]

    def g_table(self, k: int) -> Tensor:
        return self.g_tables[self.table_offsets[k]:self.table_offsets[k] + self.table_sizes[k]]

    def repack(self) -> None:
        pack(self.net, self.packed)
        ops.f32_to_f16(self.tables, self.tables_h)

    @staticmethod
    def slice_table():
        """(key, 'net', offset, shape) of every network parameter inside the flat vector (the four grids: load_from_model)"""
        return [(key, "net", off, (cnt,)) for key, off, cnt in MODULE_SLICES]

    def load_from_model(self, model) -> None:
        with torch.no_grad():
            for k, name in enumerate(GRIDS):
                self.table(k).copy_(getattr(model, name).encoding.params)
        super().load_from_model(model)

    def copy_to_model(self, model) -> None:
        super().copy_to_model(model)
        with torch.no_grad():
            for k, name in enumerate(GRIDS):
                getattr(model, name).encoding.params.copy_(self.table(k))

    def _workspace(self, n: int, which: str = "batch", train: bool = True) -> Workspace:
        """the step's workspace laid out in one grow-only buffer per use (data batch / regulariser probes); ``train=False``: the
        evaluation size, so that a render chunk of millions of samples does not grow the buffer to the training layout"""
        return Workspace(n, self.device, buf=self._buf(which, Workspace.bytes(n, train)), train=train)

    def _hash_scratch_tables(self, n: int, n_levels: int, n_tables: int) -> Tensor:
        return self._buf("hash_tables", _lib.load().nerf_hash_encode_bwd_tables_workspace_bytes(n, n_levels, n_tables))

    def _hash_scratch_probes(self, n: int, n_levels: int) -> Tensor:
        """the probes' (accumulating, counted) scatters: their own workspace -- the data batch's keep their bin estimates"""
        return self._buf("hash_probes", ops.hash_encode_bwd_workspace_bytes(n, n_levels))

    def _hash_scratch(self, n: int, n_levels: int) -> Tensor:
        return self._buf("hash", ops.hash_encode_bwd_workspace_bytes(n, n_levels))

    def _tables_for_forward(self):
        return [self.table(k, half=True).view(-1, 2) for k in range(4)]

    # -- field -----------------------------------------------------------------------------------------------
    def compute_gradients(self, rays_o: Tensor, rays_d: Tensor, target: Tensor, times: Tensor, n_samples: int, prepared=None,
                          first_ray: int = 0, bg: Optional[Tensor] = None, sync_grads_async=None, probes=None,
                          shard_grads: bool = False) -> Tensor:
        """Forward + backward of one batch: fills g_net / g_tables with the gradient of
        MSE + deformation_reg_weight * mean(mean_delta_x^2) (+ the probe regularisers) of the LOCAL rays; returns the RGB loss.
        ``sync_grads_async(view)``: data-parallel hook, called with gradient ranges as they become final."""
        R = rays_o.shape[0]
        prepared, counter = prepared if prepared is not None else self.prepare_batch(rays_o, rays_d, n_samples, first_ray)
        z, slots, pts, dirs = prepared.get()
        n = pts.shape[0]
        bg = self.bg if bg is None else bg
        self._g_net_scalars.zero_()
        # a fresh zeroed (loss, regulariser) slot per step out of a ring cleared half a lap ahead: the returned loss is a VIEW of its
        # slot (valid for the next 16384 steps) -- no copy launch per step
        row = self._loss_ring.take()
        loss, reg = row[0:1], row[1:2]
        self.last_reg = reg[0]                 # displacement regulariser of this batch (times its weight), a view like the loss
        handles = []
        reduce = (lambda view: handles.append(sync_grads_async(view))) if sync_grads_async is not None else (lambda view: None)
        if n == 0:
            self.g_tables.zero_()
            loss = ((bg.expand(R, 3) - target) ** 2).mean().reshape(1)
        else:
            ws = self._workspace(n)
            x_def, t_def = sample_inputs(slots, pts, times, R, n_samples, self.std_x, self.std_t, self.seed, counter, first_ray)
            rgb, sigma, dx, xc = forward_chain(self.packed, self.net, self._tables_for_forward(), self.levels_d, self.levels_c, self.bound,
                                               pts, x_def, t_def, dirs, ws, True)
            d_rgb, d_sigma, d_extra = composite_mse_reg_bwd(rgb, sigma, slots, z, rays_d, bg, target, dx, self.reg_weight, R, n_samples, loss,
                                                            reg, ops.sum_ws(self.device))
            g_tabs = [self.g_table(k) for k in range(4)]
            backward_chain(self.packed, self.net, self.table(3, half=True), self.levels_d, self.levels_c, self.bound, pts if x_def is None else x_def,
                           xc, ws, rgb, sigma, d_rgb, d_sigma, d_extra, self.g_net, g_tabs, hash_ws=self._hash_scratch, overwrite=True, tables_ws=self._hash_scratch_tables, extra_in_place=True,
                           spec=(self.spec_c, self.spec_d, (self.binary_grid.data_ptr(), self.binary_grid._version)),
                           after_grid=(lambda k: reduce(g_tabs[k])) if (sync_grads_async is not None and probes is None and not shard_grads) else None)
        if probes is not None:
            self._probe_regularisers(probes)
        if shard_grads and self.shard is not None:
            # sharded optimiser: ONE reduce-scatter of the flat table gradient (every rank ends with the summed gradient of its
            # slice) + the networks' small all-reduce; the same two collectives on every rank whatever its shard held
            import torch.distributed as dist
            self.shard.reduce_scatter_grads()
            if self.world_size > 1:
                dist.all_reduce(self.g_net, op=dist.ReduceOp.SUM)
        elif sync_grads_async is not None:
            if n == 0 or probes is not None:
                for k in (3, 0, 1, 2):                       # the order and sizes of the busy ranks' collectives
                    reduce(self.g_table(k))
            reduce(self.g_net)
            wait_all(handles)
        return loss[0]

    def _probe_regularisers(self, probes) -> None:
        """Temporal smoothness, unsupervised consistency and tri-grid anchor terms of the reference's loop (run.py:1861-1938)
        on their random probe points, through the SAME kernels as the data batch: one small batch of (x, t, grid weights)
        rows, deformation chain forward with stash, the terms' gradients w.r.t. delta_x as elementwise arithmetic, deformation
        chain backward accumulating into g_net / g_tables.  ``probes``: dict with any of
        temporal = (x [m,3], t [m,1], eps, weight), unsup = (x, t, weight), anchor = (x, weight)."""
        dev = self.device
        rows_x, rows_t, rows_w = [], [], []
        e = lambda k, m: torch.eye(3, device=dev)[k].expand(m, 3)
        spans = {}

        def add(name, x, t, grid):
            spans[name] = (sum(r.shape[0] for r in rows_x), x.shape[0])
            rows_x.append(x); rows_t.append(t.reshape(-1)); rows_w.append(e(grid, x.shape[0]))
        if "temporal" in probes:
            x, t, eps, _ = probes["temporal"]
            add("tmp0", x, t, 0); add("tmp1", x, t + eps, 0)
        if "unsup" in probes:
            x, t, _ = probes["unsup"]
            add("unsup", x, t, 0)
        if "anchor" in probes:
            x, _ = probes["anchor"]
            m = x.shape[0]
            add("at0", x, torch.zeros(m, device=dev), 0)
            add("a_start", x, torch.full((m,), 1.0 / 6.0, device=dev), 0)
            add("a_mid", x, torch.full((m,), 1.0 / 6.0, device=dev), 1)
        if not rows_x:
            return
        X, Tm, W = torch.cat(rows_x).contiguous(), torch.cat(rows_t).contiguous(), torch.cat(rows_w).contiguous()
        n = X.shape[0]
        ws = self._workspace(n, "probes")
        _, _, dx, _ = forward_chain(self.packed, self.net, self._tables_for_forward(), self.levels_d, self.levels_c, self.bound,
                                    X, None, Tm, None, ws, True, blend=W)
        g = torch.zeros_like(dx)
        sl = lambda name: slice(spans[name][0], spans[name][0] + spans[name][1])
        if "temporal" in probes:
            w = probes["temporal"][3] * 16
            diff = dx[sl("tmp0")] - dx[sl("tmp1")]
            g[sl("tmp0")] += 2 * w * diff / diff.numel()
            g[sl("tmp1")] -= 2 * w * diff / diff.numel()
        if "unsup" in probes:
            w = probes["unsup"][2] * 32
            d = dx[sl("unsup")]
            g[sl("unsup")] += (w / 3.0) * torch.sign(d.mean(dim=0, keepdim=True)).expand_as(d) / d.shape[0]
        if "anchor" in probes:
            w = probes["anchor"][1] * 16
            a0, a1, a2 = dx[sl("at0")], dx[sl("a_start")], dx[sl("a_mid")]
            g[sl("at0")] += 2 * w * a0 / a0.numel()
            g[sl("a_start")] += 2 * w * 0.1 * (a1 - a2) / a1.numel()
            g[sl("a_mid")] -= 2 * w * 0.1 * (a1 - a2) / a1.numel()
        backward_chain(self.packed, self.net, self.table(3), self.levels_d, self.levels_c, self.bound, X, None, ws, None, None, None, None,
                       g, self.g_net, [self.g_table(k) for k in range(4)], hash_ws=self._hash_scratch_probes)

    def enable_sharded_optimizer(self, rank: int) -> None:
        """Data parallelism as SURVEY 8(e) specifies for the big tables (project-nerf_amd/sharded.py): the table gradient is
        reduce-scattered, this rank steps its 1/world slice of the flat table buffer, the fp16 copy is all-gathered.  Call once,
        after the replicas' parameters were made equal; compute_gradients(shard_grads=True) + apply_gradients() then take this path."""
        from .sharded import ShardedTableOptimizer
        nd, nc = self.table_sizes[0], self.table_sizes[3]
        tabs = [(k * nd, nd, self.tv_disp) for k in range(3)] + [(3 * nd, nc, self.tv_canon)]
        self.shard = ShardedTableOptimizer(tabs, self.tables.numel(), rank, self.world_size, self._tables_buf, self._g_tables_buf,
                                           self._m_buf, self._v_buf, self._tables_h_buf)

    def gather_master(self) -> None:
        """sharded optimiser: bring the fp32 master copy of every slice up to date on this rank (checkpoints, validation)"""
        if self.shard is not None:
            self.shard.gather_master()

    def _apply_gradients_sharded(self) -> None:
        """apply_gradients with the table groups sharded over the ranks: this rank's slice of TV + norm and of clip + AdamW, ONE
        scalar all-reduce for the squared norm (the networks' part is added by rank 0), the networks stepped on every rank"""
        import torch.distributed as dist
        sh = self.shard
        scale = 1.0 / self.world_size
        normsq = self._normsq_ws
        sh.accumulate_normsq(normsq, scale, first=True)         # the first piece stores the norm: no zeroing launch
        if sh.rank == 0:
            normsq_flat(self.net, self.g_net, N_PARAMS, scale, normsq, first=not sh.pieces)
        if self.world_size > 1:
            dist.all_reduce(normsq[0:1], op=dist.ReduceOp.SUM)      # every rank: the same bits, hence the same clip coefficient
        lr_t, lr_n, lr_s = self.lr(2.0), self.lr(1.0), self.lr(5.0)
        self.step_count += 1
        step = self.step_count
        sh.adamw(normsq, step, lr_t, self.wd, self.max_norm, scale)
        clip_adamw_flat(self.net, self.g_net, self.state["net"], N_PARAMS, step, lr_n, self.wd, normsq, self.max_norm, scale, SCALE, lr_s)
        sh.exchange()                             # neighbours' edge elements (next step's TV terms), fp16 copy of every slice
        pack(self.net, self.packed)

    def apply_gradients(self) -> None:
        """TV-L1 on the four grids, ONE global-norm clip over every parameter (clip_grad_norm_(model.parameters()),
        run.py:1943), AdamW with the reference's group rates and cosine schedule; after a summing all-reduce the data
        gradient is averaged (1/world), the TV terms are added unscaled."""
        if self.shard is not None:
            return self._apply_gradients_sharded()
        scale = 1.0 / self.world_size
        normsq = self._normsq_ws                 # [0] the squared norm of ALL groups, [1] ticket, [2:] partials (include/nerf_hip.h)
        # pass 1 (three launches): ONE squared norm over all groups; the TV terms' signs go to a two-bit code per table entry instead
        # of into the gradient (38.5 instead of 42 bytes per parameter).  The three deformation grids (equal sizes, back to back in
        # the flat buffer) in one launch, each with its own total variation
        n_def, n_can, total = self.table_sizes[0], self.table_sizes[3], self.tables.numel()
        codes = self._tv_codes
        # the first group STORES the norm (no zeroing launch), the others add
        ops.tv_normsq_codes(self.table(0), self.g_table(0), 3 * n_def, normsq, n_tables=3, tv_weight=self.tv_disp, grad_scale=scale, codes=codes)
        ops.tv_normsq_codes(self.table(3), self.g_table(3), n_can, normsq, tv_weight=self.tv_canon, grad_scale=scale, accumulate=True,
                            codes=codes[3 * n_def // 4:])
        normsq_flat(self.net, self.g_net, N_PARAMS, scale, normsq, first=False)
        lr_t, lr_n, lr_s = self.lr(2.0), self.lr(1.0), self.lr(5.0)      # the rates of THIS step: scheduler.step() follows optimizer.step()
        self.step_count += 1
        step = self.step_count
        # pass 2 (two launches): the four grids (TV weights per range, fp16 copy written), the networks + displacement_scale (its own rate)
        ops.adamw_clip_step_tv(self.tables, self.g_tables, *self.state["tables"], total, step, lr_t, normsq, weight_decay=self.wd,
                               max_norm=self.max_norm, grad_scale=scale, codes=codes, tv=(3 * n_def, self.tv_disp, n_def, self.tv_canon, n_can),
                               shadow_f16=self.tables_h)
        clip_adamw_flat(self.net, self.g_net, self.state["net"], N_PARAMS, step, lr_n, self.wd, normsq, self.max_norm, scale, SCALE, lr_s)
        pack(self.net, self.packed)

    def train_step(self, *args, **kwargs) -> Tensor:
        return super().train_step(*args, shard_grads=self.shard is not None, **kwargs)

    # -- occupancy grid / rendering ----------------------------------------------------------------------------
    @torch.no_grad()
    def field(self, pts: Tensor, dirs: Tensor, t: Tensor):
        """(rgb, sigma, delta_x) at points with per-point times, evaluation mode (no noise)"""
        n = pts.shape[0]
        ws = self._workspace(n, train=False)
        rgb, sigma, dx, _ = forward_chain(self.packed, self.net, self._tables_for_forward(), self.levels_d, self.levels_c, self.bound,
                                          pts.contiguous(), None, t.reshape(-1).contiguous(), dirs.contiguous(), ws, False)
        return rgb, sigma, dx

    @torch.no_grad()
    def update_grid(self, decay: float = 0.95, chain: bool = False) -> float:
        """DensityGrid.update of mode part4 (reference src/renderer.py:65-86, 122-125): density on the lattice at the time
        anchors 0, 0.5, 1, element-wise maximum, running maximum against the decayed history.  ``chain=True``: the refresh as ONE
        density-only launch chain (nerf_p4_grid_update) -- no lattice tensor, one deformation gather per anchor instead of three,
        no colour-net, one workspace kept on the engine; the same bits as the loop."""
        if chain:
            return self._update_grid_chain(decay)
        res = self.grid.shape[0]
        lattice = self._lattice()
        sig = torch.zeros(res ** 3, device=self.device)
        for anchor in (0.0, 0.5, 1.0):
            for i, s in self.lattice_density(lattice, anchor):
                torch.maximum(sig[i:i + s.shape[0]], s, out=sig[i:i + s.shape[0]])
        self.binary_grid, ratio = ops.grid_threshold(sig.view(res, res, res), self.grid_threshold, prev=self.grid, decay=decay)
        return ratio

    _GRID_SLAB = 2 ** 18       # cells per slab of the chain refresh: the loop form's batch

    def _update_grid_chain(self, decay: float) -> float:
        # NEW grid tensors, allocated while the old ones are alive: the speculative hash backward recognises a refresh by
        # (data_ptr, _version) of binary_grid, and a raw kernel store into the old tensor would change neither
        return grid_update_chain(                        # its one host sync the loop form also has
            self, lambda slab, ws: ops.p4_grid_update(self.packed, self.net, self._tables_for_forward(), self.levels_d, self.levels_c,
                                                      self.bound, self.grid.shape[0], self.grid_bound, self.grid_threshold,
                                                      self.grid.clone(), decay, slab_cells=slab, workspace=ws),
            ops.p4_grid_update_workspace_bytes)
