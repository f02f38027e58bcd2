"""Part 1 (2-D image fit, mode part1_fourier) as a flat-parameter training engine on one fused HIP chain: the loop body of
reference run_part1 (run.py:178-190) with NeuralField('part1_fourier') (src/core.py:25-34).

    coords[idx] -> Fourier code in registers -> Linear/ReLU x num_layers -> Linear -> sigmoid -> MSE + its derivative
    (csrc/p1fit.hip, one kernel) -> transposed chain -> weight gradients by chunk-partial MFMA tiles + one ordered reduction
    -> Adam (ops.adam_step, torch.optim.Adam's defaults) -> repack.

No torch autograd, torch.optim or library GEMM in the step.  The flat vector is the module's state dict concatenated
(decoder.net.{0,2,...}.{weight,bias}), so checkpoints keep the reference's keys.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, flat_params, ops
from .flat_engine import FlatAdamEngine

Tensor = torch.Tensor
P = ops._p

HIDDEN = (64, 128, 256)
MAX_LAYERS, MAX_L = 8, 15


def _shape(cfg: dict) -> Tuple[int, int, int, int]:
    """(L_embed, use_pe, hidden_dim, num_layers) as NeuralField reads them (src/core.py:22-28)"""
    use_pe = bool(cfg.get("use_positional_encoding", True))
    L = int(cfg.get("L_embed", 0)) if use_pe else 0
    return L, int(use_pe), int(cfg["hidden_dim"]), int(cfg.get("num_layers", 3))


def supported(cfg: dict) -> Optional[str]:
    """None if the fused chain is compiled for this configuration, else the reason it is not."""
    if cfg.get("mode") != "part1_fourier":
        return f"mode={cfg.get('mode')} (compiled: part1_fourier)"
    for key in ("L_embed", "hidden_dim", "num_layers", "use_positional_encoding"):
        if isinstance(cfg.get(key), (list, tuple)):
            return f"{key}={cfg.get(key)} (compiled: one value)"
    if cfg.get("hidden_dim") not in HIDDEN:
        return f"hidden_dim={cfg.get('hidden_dim')} (compiled: 64, 128, 256)"
    layers, L = cfg.get("num_layers", 3), cfg.get("L_embed", 0)
    if not isinstance(layers, int) or not 1 <= layers <= MAX_LAYERS:
        return f"num_layers={layers} (compiled: 1..{MAX_LAYERS})"
    if cfg.get("use_positional_encoding", True) and (not isinstance(L, int) or not 0 <= L <= MAX_L):
        return f"L_embed={L} (compiled: 0..{MAX_L})"
    if cfg.get("output_dim", 3) != 3:
        return f"output_dim={cfg.get('output_dim')} (compiled: 3)"
    return None


def slice_table(cfg: dict) -> flat_params.Table:
    """(state-dict key, offset into the flat vector, shape) of every parameter of NeuralField(cfg), in state-dict order"""
    L, _, H, layers = _shape(cfg)
    shapes, fan_in = [], 2 + 4 * L
    for i in range(layers + 1):
        out = H if i < layers else 3
        shapes += [(f"decoder.net.{2 * i}.weight", (out, fan_in)), (f"decoder.net.{2 * i}.bias", (out,))]
        fan_in = H
    return flat_params.table_of(shapes)


param_count, flatten, unflatten, default_init = flat_params.bind(slice_table)       # each takes cfg first


class Part1Engine(FlatAdamEngine):
    """Flat-parameter training / inference engine of mode part1_fourier (module docstring)."""
    RING = 1024

    def __init__(self, cfg: dict, params: Optional[Tensor] = None, device: str = "cuda", lr: float = 1e-3, seed: int = 0):
        why = supported(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Part 1 chain is not compiled for {why}")
        self.cfg = dict(cfg)
        self.shape = _shape(cfg)
        lib = _lib.load()
        super().__init__("Part 1", slice_table(cfg), lib.nerf_p1_param_count(*self.shape), lib.nerf_p1_packed_bytes(*self.shape),
                         default_init(cfg, seed) if params is None else params, device, lr)
        self._losses = torch.zeros(self.RING, device=self.device)       # one slot per step: no memset, no host sync
        self._calls = 0
        self.repack()

    # -- weights -------------------------------------------------------------------------------------------------
    def repack(self) -> None:
        _lib.check(_lib.load().nerf_p1_pack(P(self.params), *self.shape, P(self.packed), ops._stream()), "nerf_p1_pack")

    def _workspace_bytes(self, n: int) -> int:
        return _lib.load().nerf_p1_workspace_bytes(n, *self.shape)

    # -- step ----------------------------------------------------------------------------------------------------
    def compute_gradients(self, coords: Tensor, target: Tensor, idx: Optional[Tensor] = None) -> Tensor:
        """Fills ``grads`` with the gradient of mean((field(coords[idx]) - target[idx])^2) and returns the loss (a device
        scalar).  ``idx``: int64 rows (repeats allowed), or None for every row."""
        coords, target = ops._dev(coords, "coords"), ops._dev(target, "target")
        if coords.dim() != 2 or coords.shape[1] != 2 or target.shape != (coords.shape[0], 3):
            raise ValueError(f"coords [N,2] and target [N,3] expected, got {tuple(coords.shape)} and {tuple(target.shape)}")
        if idx is not None:
            idx = ops._dev(idx.reshape(-1), "idx", torch.int64)
        n = coords.shape[0] if idx is None else idx.numel()
        if n == 0:
            raise ValueError("empty batch")
        slot = self._calls % self.RING
        self._calls += 1
        loss = self._losses[slot:slot + 1]
        _lib.check(_lib.load().nerf_p1_fwd_loss_bwd(P(self.packed), P(self._workspace(n)), P(coords), P(idx), P(target), n, *self.shape,
                                                    P(self.grads), P(loss), ops._stream()), "nerf_p1_fwd_loss_bwd")
        return loss[0]

    @torch.no_grad()
    def predict(self, coords: Tensor) -> Tensor:
        coords = ops._dev(coords, "coords")
        n = coords.shape[0]
        y = torch.empty(n, 3, device=self.device)
        _lib.check(_lib.load().nerf_p1_fwd(P(self.packed), P(coords), n, *self.shape, P(y), ops._stream()), "nerf_p1_fwd")
        return y
