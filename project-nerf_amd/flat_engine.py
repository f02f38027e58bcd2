"""What the flat-parameter engines of the static modes share on the host side (part1.Part1Engine, part2.Part2Engine,
engine.VanillaNerfEngine, engine.InstantNgpEngine): the cosine rate, the chunk loop of render_image, the two policies for
"a zeroed device scalar per step without a memset launch", and the base of the engines that keep one flat vector under Adam.
It is to these what dynamic_engine.py is to the dynamic modes (which takes the rate, the loop and the slot ring from here)."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib, flat_params, ops

Tensor = torch.Tensor


def cosine_lr(base: float, eta_min: float, step: int, t_max: int) -> float:
    """torch's CosineAnnealingLR in closed form: the rate of step ``step`` of a group whose initial rate is ``base``"""
    return eta_min + (base - eta_min) * (1 + math.cos(math.pi * step / t_max)) / 2


def grid_refresh_due(step: int, iters: int, warm: int, stop: float = 0.9) -> bool:
    """Whether a training loop that goes through its occupancy grid refreshes the grid AFTER step ``step`` (1-based) of ``iters``:
    the first refresh after step ``warm`` (the steps up to it are dense), then the reference's schedule (run.py:621-627) -- every
    32 steps in the first tenth of the run, every 128 up to half of it, every 512 after that, none from ``stop`` * iters on."""
    if step < max(warm, 1):
        return False
    if step == max(warm, 1):
        return True
    if step >= iters * stop:
        return False
    interval = 32 if step < iters * 0.1 else (128 if step < iters * 0.5 else 512)
    return step % interval == 0


def render_chunks(render_rays, rays_o: Tensor, rays_d: Tensor, chunk: int, device) -> Tensor:
    """[..., 3] colours of rays [..., 3]: ``render_rays(o, d)[0]`` over ``chunk`` rays at a time"""
    shape = rays_o.shape[:-1]
    o, d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    out = torch.empty(o.shape[0], 3, device=device)
    for i in range(0, o.shape[0], chunk):
        out[i:i + chunk] = render_rays(o[i:i + chunk], d[i:i + chunk])[0]
    return out.view(*shape, 3)


def render_counted_chain(render, workspace_bytes, kept: Dict, rays_o: Tensor, rays_d: Tensor, n_samples: int, chunk: int, device) -> Tensor:
    """[..., 3] colours of rays [..., 3] through a counted render chain (ops.render_rays_grid_fwd, ops.instant_render_rays_fwd):
    ``render(o, d, chunk, workspace)[0]`` for all rays in one call, ``chunk`` clamped to [1, number of rays], ONE workspace of
    ``workspace_bytes(chunk, n_samples)`` bytes kept in ``kept`` per (chunk, n_samples)"""
    shape = rays_o.shape[:-1]
    o, d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    chunk = max(1, min(int(chunk), max(o.shape[0], 1)))
    ws = kept.get((chunk, n_samples))
    if ws is None:
        ws = kept[(chunk, n_samples)] = torch.empty(workspace_bytes(chunk, n_samples), dtype=torch.uint8, device=device)
    return render(o, d, chunk, ws)[0].view(*shape, 3)


def grid_update_chain(engine, refresh, workspace_bytes) -> float:
    """The active ratio after an occupancy-grid refresh as a density-only launch chain (ops.instant_grid_update, ops.p4_grid_update,
    ops.p3_grid_update): ``refresh(slab_cells, workspace)`` over slabs of ``engine._GRID_SLAB`` cells, ONE workspace of
    ``workspace_bytes(slab_cells)`` bytes kept in ``engine._grid_ws``; its (grid, binary_grid) become the engine's.  They are
    installed BEFORE the one host read of the count: the tensors they replace are released while the device is still busy, not
    between the read and the next refresh, where nothing hides the time (measured: 4 us of a 0.79 ms refresh)."""
    ws = engine._grid_ws
    if ws is None:
        ws = engine._grid_ws = torch.empty(workspace_bytes(engine._GRID_SLAB), dtype=torch.uint8, device=engine.device)
    engine.grid, engine.binary_grid, count = refresh(engine._GRID_SLAB, ws)
    return float(count.item()) / engine.binary_grid.numel()


# --------------------------------------------------------------------------------------------------- per-step scalar slots
class ViewSlots:
    """A fresh zeroed row per call out of a zeroed ring [slots, width], with no fill launch and no copy launch per step: the row
    handed out is a VIEW, valid for the next slots / 2 calls.  Entering a half of the ring clears that half, whose rows were
    handed out at least half a lap ago; call 0 clears nothing (the ring comes zeroed)."""

    def __init__(self, ring: Tensor):
        self.ring, self.calls = ring, 0

    def take(self) -> Tensor:
        n = self.ring.shape[0]
        slot = self.calls % n
        if slot % (n // 2) == 0 and self.calls > 0:
            self.ring[slot:slot + n // 2].zero_()
        self.calls += 1
        return self.ring[slot]


class LapSlots:
    """A fresh zeroed column per call out of a ring [rows, slots] that is cleared once per lap, instead of a memset launch per
    step.  ``take()`` hands out one one-element view per row; what a caller may hold on to is ``keep(view)``, a COPY that the
    next lap's clear does not reach."""

    def __init__(self, ring: Tensor):
        self.ring, self.rows, self.calls = ring, ring.unbind(0), 0

    def take(self):
        slot = self.calls % self.ring.shape[1]
        self.calls += 1
        if slot == 0:
            self.ring.zero_()
        return [row[slot:slot + 1] for row in self.rows]

    @staticmethod
    def keep(view: Tensor) -> Tensor:
        return view[0].clone()


# --------------------------------------------------------------------------------------------------- engines
class FlatAdamEngine:
    """State and methods common to the engines that train one flat fp32 vector (a module's state dict concatenated over a slice
    table) with torch.optim.Adam's defaults and keep packed fragment images of it.  A subclass checks its configuration, sets
    ``cfg`` and ``shape``, hands its table and the library's two sizes to __init__, defines repack, _workspace_bytes and
    compute_gradients, and calls repack() last in its own __init__."""

    def __init__(self, what: str, table: flat_params.Table, lib_count: int, packed_bytes: int, params: Tensor, device: str, lr: float):
        self.slices = table
        self.device = torch.device(device)
        n = flat_params.param_count(table)
        if lib_count != n:
            raise _lib.NerfHipError(f"libnerf_hip.so reports {lib_count} {what} parameters, this binding expects {n}")
        flat = params.detach().float().reshape(-1)
        if flat.numel() != n:
            raise ValueError(f"{what} engine: {n} parameters expected, got {flat.numel()}")
        self.params = flat.to(self.device).contiguous().clone()
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.packed = torch.empty(packed_bytes, dtype=torch.uint8, device=self.device)
        self.lr = float(lr)
        self.step_count = 0
        self._ws: Optional[Tensor] = None

    # -- weights -------------------------------------------------------------------------------------------------
    def load_from_model(self, model) -> None:
        with torch.no_grad():
            self.params.copy_(flat_params.flatten(self.slices, model.state_dict()).to(self.device))
        self.repack()

    def copy_to_model(self, model) -> None:
        state = model.state_dict()                     # references to the module's tensors (buffers such as freq_bands stay)
        with torch.no_grad():
            for k, v in flat_params.unflatten(self.slices, self.params).items():
                state[k].copy_(v)

    def state_dict(self, prefix: str = "decoder.") -> Dict[str, Tensor]:
        return {prefix + k[len("decoder."):]: v.clone() for k, v in flat_params.unflatten(self.slices, self.params).items()}

    def _workspace(self, n: int) -> Tensor:
        need = self._workspace_bytes(n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)        # grow-only
        return self._ws

    # -- step ----------------------------------------------------------------------------------------------------
    def apply_gradients(self) -> None:
        """torch.optim.Adam's defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay), then the fragment images again"""
        self.step_count += 1
        ops.adam_step(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr)
        self.repack()

    def train_step(self, *args, **kwargs) -> Tensor:
        """compute_gradients (the arguments are its own) then apply_gradients; returns the loss"""
        loss = self.compute_gradients(*args, **kwargs)
        self.apply_gradients()
        return loss
