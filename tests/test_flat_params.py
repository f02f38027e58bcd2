"""Host side of what the static-field engines share (project-nerf_amd/flat_params.py, flat_engine.py), no GPU and no library:
the slice tables and default initialisations pinned bit for bit, the three spellings of the NeRF decoder's parameter list
held to one table, and the two per-step scalar-slot policies walked over three laps of a small ring on CPU tensors."""
import hashlib

import pytest
import torch

from project_nerf_amd import engine, flat_engine, flat_params, part1, part2, part3_nerf


def part1_cfg(H, layers, L):
    return {"mode": "part1_fourier", "use_positional_encoding": True, "L_embed": L, "hidden_dim": H, "num_layers": layers}


def part2_cfg(H, layers, skip, V, L, Ld):
    return {"mode": "part2_nerf", "use_positional_encoding": True, "L_embed": L, "use_viewdirs": True, "L_embed_dir": Ld,
            "hidden_dim": H, "num_layers": layers, "skip_layer": skip, "view_dim": V}


P2_DEFAULT = part2_cfg(256, 8, 4, 128, 10, 4)
P2_SMALLEST = part2_cfg(64, 2, 1, 64, 1, 0)            # the smallest shape the chain is compiled for
P1_PLAIN, P1_WIDEST_CODE = part1_cfg(64, 1, 0), part1_cfg(64, 1, 15)


def table_digest(rows) -> str:
    """SHA-256 of the (key, offset, shape) list as plain Python values"""
    return hashlib.sha256(repr([(str(k), int(off), tuple(int(s) for s in shape)) for k, off, shape in rows]).encode()).hexdigest()


def tensor_digest(t: torch.Tensor) -> str:
    assert t.dtype == torch.float32 and t.dim() == 1
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def with_offsets(shapes):
    """engine.param_shapes() carries no offsets: the running sum, as its flatten lays the vector out"""
    rows, off = [], 0
    for key, shape in shapes:
        rows.append((key, off, shape))
        off += int(torch.Size(shape).numel())
    return rows


CASES = {
    "engine": (lambda: with_offsets(engine.param_shapes()), lambda seed: engine.default_init(seed)),
    "part2-default": (lambda: part2.slice_table(P2_DEFAULT), lambda seed: part2.default_init(P2_DEFAULT, seed)),
    "part2-smallest": (lambda: part2.slice_table(P2_SMALLEST), lambda seed: part2.default_init(P2_SMALLEST, seed)),
    "part1-L0": (lambda: part1.slice_table(P1_PLAIN), lambda seed: part1.default_init(P1_PLAIN, seed)),
    "part1-L15": (lambda: part1.slice_table(P1_WIDEST_CODE), lambda seed: part1.default_init(P1_WIDEST_CODE, seed)),
}

# (table, default_init(0), default_init(3)) digests printed by this file's own functions at commit ded7877, the last one before
# the tables and helpers were shared: engine.default_init divides by fan_in ** 0.5, Part 1 and Part 2 multiply by
# 1 / sqrt(fan_in), and the two differ in the last bit -- which is why "engine" and "part2-default" share a table but no vector
EXPECTED = {
    "engine": ("5c9939c756b6b6101f97952f60382ed8db8e3d3955422acbf801c5fd96dcc987", "7fafd2f8d4bdfe2b6c509b0910f5dcdfa156efb3ffc6035a3f8e61047c20f1e1", "621fb68b3620369ceb4519f375fc140c34cadb3f0d81457682a6d167cc95ec4f"),
    "part2-default": ("998b296f096c8c2c32bf93d64bfa62aa05e85d107ae721f151626b61d5542d55", "b3600d56930301e6fb6c1741a748a99f1c07967d8e5769968a511083cf7b1ac1", "3bd8f77521266a21f94515091ca3c22e2818f2980356713ca6d7133fd2938c8c"),
    "part2-smallest": ("bd7029b98822f2c148e0f85b190678b4d9d9cbcd9c6a1756d2184f6b87812bc1", "94372bfdbfe9dfe9342032ff2241d3953103dc0881114406b64e4102d4e5612c", "74c8e297f47cfa93275685a7729e4b481b9945e9681ce56287edb948613750eb"),
    "part1-L0": ("7165c857a3c15d522c85153beb26a7c08b3cc0fd66981b6955b5d4c609639ff5", "451abd3e09dc4fd4b84a5a4a58b9c6da8994e1de849f5848879cf9a736ad80e3", "01b76c9e5c4dea8e9b3df0bade74fd83a9b47e02f3904e413b6c4bd9a1243e84"),
    "part1-L15": ("a1ab037c7fd1a7dd9e76bc5159bbbc3634c51ab01b2cf338f429e2d90e8cedd4", "6ef1d4392d0459a710a6189d571c0e00cc43879899d04fb9d6cc5058c7760f85", "a86bf7438c3ca5c35f6774a6ded1a1aab503f07376e9f705f356f771706a3752"),
}


def actual(name):
    table, init = CASES[name]
    return table_digest(table()), tensor_digest(init(0)), tensor_digest(init(3))


@pytest.mark.parametrize("name", list(CASES))
def test_table_and_default_init_bits_are_those_of_the_unshared_code(name):
    got = actual(name)
    print(name, got)
    assert got == EXPECTED[name]


def test_the_three_decoder_tables_are_one_table():
    """engine.param_shapes, part2.slice_table at the default shape and part3_nerf.decoder_shapes("decoder", 63) are derived from
    flat_params.nerf_decoder_table; editing one of them alone breaks this"""
    shared = flat_params.nerf_decoder_table("decoder.", 63, 27, 256, 8, 4, 128)
    assert part2.slice_table(P2_DEFAULT) == shared
    assert [("decoder." + k, s) for k, s in engine.param_shapes()] == [(k, s) for k, _, s in shared]
    assert part3_nerf.decoder_shapes("decoder", 63) == [(k, s) for k, _, s in shared]
    assert flat_params.param_count(shared) == part2.param_count(P2_DEFAULT) == engine.default_init(0).numel() == 595844
    # and the decoder Part 3 trains (its time code appended to the position code) is the same function at another width
    wide = flat_params.nerf_decoder_table("decoder_direct.", 63 + 21, 27, 256, 8, 4, 128)
    assert part3_nerf.decoder_shapes("decoder_direct", 84) == [(k, s) for k, _, s in wide]


def test_generic_helpers_round_trip_over_a_table():
    table = part2.slice_table(P2_SMALLEST)
    flat = torch.arange(flat_params.param_count(table), dtype=torch.float32)
    parts = flat_params.unflatten(table, flat)
    assert list(parts) == [k for k, _, _ in table]
    assert all(parts[k].shape == tuple(s) and parts[k].reshape(-1)[0] == off for k, off, s in table)
    assert torch.equal(flat_params.flatten(table, parts), flat)
    assert torch.equal(part2.flatten(P2_SMALLEST, parts), flat) and torch.equal(part1.default_init(P1_PLAIN, 3), flat_params.linear_init(part1.slice_table(P1_PLAIN), 3))


# ---------------------------------------------------------------------------------------------- per-step scalar slots
SLOTS, LAPS = 8, 3


def test_view_slots_clear_half_a_lap_behind_and_never_on_call_0():
    ring = torch.full((SLOTS, 2), 7.0)                 # call 0 clears nothing: the ring must come zeroed, this one does not
    slots = flat_engine.ViewSlots(ring)
    assert torch.equal(slots.take(), torch.full((2,), 7.0)) and torch.equal(ring, torch.full((SLOTS, 2), 7.0))
    ring.zero_()
    slots = flat_engine.ViewSlots(ring)
    held = []
    for call in range(LAPS * SLOTS):
        row = slots.take()
        assert row.shape == (2,) and row.data_ptr() == ring[call % SLOTS].data_ptr()        # a view of its slot
        assert torch.equal(row, torch.zeros(2)), call                                       # exactly 0.0 when handed out
        row += 1.0                                                                           # the kernel's accumulation
        held.append(row)
        if call >= 3:                                  # 3 calls later is inside the half lap of 4 for which a view stays valid
            assert torch.equal(held[call - 3], torch.ones(2)), call
    assert slots.calls == LAPS * SLOTS


def test_lap_slots_clear_once_per_lap_and_hand_back_a_copy():
    ring = torch.zeros(2, SLOTS)
    slots = flat_engine.LapSlots(ring)
    kept = []
    for call in range(LAPS * SLOTS):
        loss, amax = slots.take()
        assert loss.shape == (1,) and loss.data_ptr() == ring[0, call % SLOTS:].data_ptr() and amax.data_ptr() == ring[1, call % SLOTS:].data_ptr()
        assert float(loss) == 0.0 and float(amax) == 0.0, call                              # exactly 0.0 when handed out
        loss += 1.0
        amax += 1.0
        kept.append(flat_engine.LapSlots.keep(loss))
        assert kept[-1].dim() == 0 and kept[-1].data_ptr() != loss.data_ptr()
    assert all(float(k) == 1.0 for k in kept)          # every returned value survived the clears of the two later laps
    assert slots.calls == LAPS * SLOTS
