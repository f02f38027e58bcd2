"""Flat parameter vectors over a slice table, once for every engine that keeps a module's state dict concatenated.

A slice table is a list of (state-dict key, offset into the flat vector, shape), in state-dict order.  The generic helpers take
a table; each engine module binds them to its own table function, so ``part1.flatten(cfg, state)`` and its like keep their
signatures.  The NeRF decoder's table stands here as well, because three modules spell that one list: engine.param_shapes,
part2.slice_table and part3_nerf.decoder_shapes are derived from ``nerf_decoder_table``.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import torch

Tensor = torch.Tensor
Table = List[Tuple[str, int, Tuple[int, ...]]]


def table_of(shapes: Sequence[Tuple[str, Tuple[int, ...]]]) -> Table:
    """(key, shape) in state-dict order -> (key, offset, shape): the parameters tile the flat vector with no gaps"""
    table, off = [], 0
    for key, shape in shapes:
        table.append((key, off, shape))
        off += math.prod(shape)
    return table


def param_count(table: Table) -> int:
    key, off, shape = table[-1]
    return off + math.prod(shape)


def flatten(table: Table, state: Dict[str, Tensor]) -> Tensor:
    return torch.cat([state[k].detach().float().reshape(-1) for k, _, _ in table])


def unflatten(table: Table, flat: Tensor) -> Dict[str, Tensor]:
    return {k: flat[off:off + math.prod(shape)].view(shape) for k, off, shape in table}


def linear_init(table: Table, seed: int = 0) -> Tensor:
    """nn.Linear's default initialisation (weights and biases uniform in +-1/sqrt(fan_in)) of every layer, flat"""
    g = torch.Generator().manual_seed(seed)
    flat = torch.empty(param_count(table))
    fan_in = {k: shape[1] for k, _, shape in table if k.endswith("weight")}
    for key, off, shape in table:
        bound = 1.0 / math.sqrt(fan_in[key.replace("bias", "weight")])       # a bias takes its layer's fan-in
        n = math.prod(shape)
        flat[off:off + n] = (torch.rand(n, generator=g) * 2 - 1) * bound
    return flat


def bind(slice_table):
    """(param_count, flatten, unflatten, default_init) of a module whose ``slice_table(cfg)`` gives its table: the helpers above
    with the configuration in the table's place, as part1 and part2 export them"""
    def _param_count(cfg: dict) -> int:
        return param_count(slice_table(cfg))

    def _flatten(cfg: dict, state: Dict[str, Tensor]) -> Tensor:
        return flatten(slice_table(cfg), state)

    def _unflatten(cfg: dict, flat: Tensor) -> Dict[str, Tensor]:
        return unflatten(slice_table(cfg), flat)

    def _default_init(cfg: dict, seed: int = 0) -> Tensor:
        return linear_init(slice_table(cfg), seed)
    return _param_count, _flatten, _unflatten, _default_init


def nerf_decoder_table(prefix: str, pos_dim: int, dir_dim: int, hidden: int = 256, layers: int = 8, skip: int = 4,
                       view: int = 128) -> Table:
    """NeRFDecoder(pos_dim, dir_dim, hidden, layers, skip, view) in registration order (reference src/decoders.py:37-66): the
    position code enters layer 0 and again, next to the hidden vector, layer ``skip``.  ``prefix`` is put in front of every key
    as it is ("decoder." for the module's state dict, "" for the bare decoder)."""
    shapes = []
    for i in range(layers):
        k = pos_dim if i == 0 else hidden
        if i == skip:
            k += pos_dim
        shapes.append((f"pts_layers.{i}", (hidden, k)))
    shapes += [("sigma_layer", (1, hidden)), ("feature_layer", (hidden, hidden)), ("view_layer", (view, hidden + dir_dim)),
               ("rgb_layer", (3, view))]
    rows = []
    for name, shape in shapes:
        rows += [(f"{prefix}{name}.weight", shape), (f"{prefix}{name}.bias", shape[:1])]
    return table_of(rows)
