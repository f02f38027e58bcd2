"""Part 1 (2-D image fit, mode part1_fourier) as a flat-parameter training engine on one fused HIP chain: the loop body of
reference run_part1 (run.py:178-190) with NeuralField('part1_fourier') (src/core.py:25-34).

    coords[idx] -> Fourier code in registers -> Linear/ReLU x num_layers -> Linear -> sigmoid -> MSE + its derivative
    (csrc/p1fit.hip, one kernel) -> transposed chain -> weight gradients by chunk-partial MFMA tiles + one ordered reduction
    -> Adam (ops.adam_step, torch.optim.Adam's defaults) -> repack.

No torch autograd, torch.optim or library GEMM in the step.  The flat vector is the module's state dict concatenated
(decoder.net.{0,2,...}.{weight,bias}), so checkpoints keep the reference's keys.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

Tensor = torch.Tensor
P = lambda t: None if t is None else t.data_ptr()

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


def slice_table(cfg: dict) -> List[Tuple[str, int, Tuple[int, ...]]]:
    """(state-dict key, offset into the flat vector, shape) of every parameter of NeuralField(cfg), in state-dict order"""
    L, _, H, layers = _shape(cfg)
    table, off = [], 0
    fan_in = 2 + 4 * L
    for i in range(layers + 1):
        out = H if i < layers else 3
        for name, shape in (("weight", (out, fan_in)), ("bias", (out,))):
            table.append((f"decoder.net.{2 * i}.{name}", off, shape))
            off += math.prod(shape)
        fan_in = H
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


class Part1Engine:
    """Flat-parameter training / inference engine of mode part1_fourier (module docstring)."""
    RING = 1024

    def __init__(self, cfg: dict, params: Optional[Tensor] = None, device: str = "cuda", lr: float = 1e-3, seed: int = 0):
        from . import _lib
        why = supported(cfg)
        if why is not None:
            raise NotImplementedError(f"the fused Part 1 chain is not compiled for {why}")
        self.cfg = dict(cfg)
        self.shape = _shape(cfg)
        self.device = torch.device(device)
        lib = _lib.load()
        n = lib.nerf_p1_param_count(*self.shape)
        if n != param_count(cfg):
            raise _lib.NerfHipError(f"libnerf_hip.so reports {n} Part 1 parameters, this binding expects {param_count(cfg)}")
        flat = default_init(cfg, seed) if params is None else params.detach().float().reshape(-1)
        if flat.numel() != n:
            raise ValueError(f"Part 1 engine: {n} parameters expected, got {flat.numel()}")
        self.params = flat.to(self.device).contiguous().clone()
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.packed = torch.empty(lib.nerf_p1_packed_bytes(*self.shape), dtype=torch.uint8, device=self.device)
        self.lr = float(lr)
        self.step_count = 0
        self._ws: Optional[Tensor] = None
        self._losses = torch.zeros(self.RING, device=self.device)       # one slot per step: no memset, no host sync
        self._calls = 0
        self.repack()

    # -- weights -------------------------------------------------------------------------------------------------
    def repack(self) -> None:
        from . import _lib, ops
        _lib.check(_lib.load().nerf_p1_pack(P(self.params), *self.shape, P(self.packed), ops._stream()), "nerf_p1_pack")

    def load_from_model(self, model) -> None:
        with torch.no_grad():
            self.params.copy_(flatten(self.cfg, model.state_dict()).to(self.device))
        self.repack()

    def copy_to_model(self, model) -> None:
        state = model.state_dict()                     # references to the module's tensors (buffers such as freq_bands stay)
        with torch.no_grad():
            for k, v in unflatten(self.cfg, self.params).items():
                state[k].copy_(v)

    def _workspace(self, n: int) -> Tensor:
        from . import _lib
        need = _lib.load().nerf_p1_workspace_bytes(n, *self.shape)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)        # grow-only
        return self._ws

    # -- step ----------------------------------------------------------------------------------------------------
    def compute_gradients(self, coords: Tensor, target: Tensor, idx: Optional[Tensor] = None) -> Tensor:
        """Fills ``grads`` with the gradient of mean((field(coords[idx]) - target[idx])^2) and returns the loss (a device
        scalar).  ``idx``: int64 rows (repeats allowed), or None for every row."""
        from . import _lib, ops
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

    def apply_gradients(self) -> None:
        """torch.optim.Adam's defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay), then the fragment images again"""
        from . import ops
        self.step_count += 1
        ops.adam_step(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr)
        self.repack()

    def train_step(self, coords: Tensor, target: Tensor, idx: Optional[Tensor] = None) -> Tensor:
        loss = self.compute_gradients(coords, target, idx)
        self.apply_gradients()
        return loss

    @torch.no_grad()
    def predict(self, coords: Tensor) -> Tensor:
        from . import _lib, ops
        coords = ops._dev(coords, "coords")
        n = coords.shape[0]
        y = torch.empty(n, 3, device=self.device)
        _lib.check(_lib.load().nerf_p1_fwd(P(self.packed), P(coords), n, *self.shape, P(y), ops._stream()), "nerf_p1_fwd")
        return y
