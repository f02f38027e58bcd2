"""nerf_train_batch_compact / nerf_train_batch_compact_chain -- the data side of a training step through the occupancy grid in one
launch -- against the two calls it replaces on the same (seed, counter, first_ray): nerf_train_batch_shard for the rays and
targets, nerf_sample_compact_jitter_shard (fed those rays) for depths, active mask, count and compact rows.  Everything is
torch.equal: the kernel restates the same separately rounded operations; only the slot ORDER is arbitrary (in both), so compact
rows are compared through each call's own slot map.  Frames are [3, 8, 8, 4], the grid is 8^3: each case runs in well under a
second."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NEAR, FAR, BOUND, RES, SEED = 2.0, 6.0, 1.5, 8, 11
# (batch, n_samples, first_ray)
CASES = {"smallest": (1, 2, 0), "one-pass": (64, 64, 0), "4095-straddle": (63, 65, 0), "4097-second-pass": (241, 17, 0),
         "several-workgroups-shard": (700, 64, 1300),
         # 4,194,432 samples: one pass more than the 1024-workgroup cap covers, so workgroup 0 takes a second, ragged trip of the
         # grid-stride loop (the smallest such count); the "seeded" grid only
         "past-the-workgroup-cap": (32769, 128, 0)}
GRIDS = ("ones", "zeros", "seeded")
PLAIN_FORM = [(case, kind) for case in CASES for kind in GRIDS if case != "past-the-workgroup-cap" or kind == "seeded"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from project_nerf_amd import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from project_nerf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def scene():
    """three random RGBA frames with random rigid poses: cameras on the sphere of radius 4 looking at the box (so that rays enter and
    leave it between near and far), rolled about their axis"""
    g = torch.Generator().manual_seed(5)
    images = torch.rand(3, 8, 8, 4, generator=g)
    poses = torch.zeros(3, 4, 4)
    for i in range(3):
        pos = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0) * 4.0
        back = pos / pos.norm()
        right = torch.nn.functional.normalize(torch.cross(torch.randn(3, generator=g), back, dim=0), dim=0)
        up = torch.cross(back, right, dim=0)
        poses[i, :3, 0], poses[i, :3, 1], poses[i, :3, 2], poses[i, :3, 3] = right, up, back, pos + 0.2 * torch.randn(3, generator=g)
        poses[i, 3, 3] = 1.0
    return images.cuda().contiguous(), poses.cuda().contiguous(), 5.5, torch.tensor([1.0, 0.5, 0.25]).cuda()


def make_grid(kind):
    if kind == "ones":
        return torch.ones(RES, RES, RES, dtype=torch.bool, device="cuda")
    if kind == "zeros":
        return torch.zeros(RES, RES, RES, dtype=torch.bool, device="cuda")
    return (torch.rand(RES, RES, RES, generator=torch.Generator().manual_seed(3)) < 0.3).cuda()


def filled(*shape, dtype=torch.float32):
    """a tensor whose every byte is 0xFF"""
    t = torch.empty(*shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def is_filled(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


P = lambda t: None if t is None else t.data_ptr()
_REFERENCE = {}


def reference(ops, lib, scene, case, kind):
    """the two calls the kernel replaces, computed once per (case, grid) and left unchanged"""
    key = (case, kind)
    if key not in _REFERENCE:
        images, poses, focal, bg = scene
        batch, S, first = CASES[case]
        counter = 7 + len(case)
        o, d, target, _ = ops.train_batch(images, poses, focal, batch, S, NEAR, FAR, SEED, counter, bg=bg, first_ray=first)
        o2, d2, rgba, _ = ops.train_batch(images, poses, focal, batch, S, NEAR, FAR, SEED, counter, first_ray=first)
        assert torch.equal(o, o2) and torch.equal(d, d2)
        grid = make_grid(kind)
        n = batch * S
        z, slots = filled(batch, S), filled(n, dtype=torch.int32)
        pts, dirs = filled(n, 3), filled(n, 3)
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.nerf_sample_compact_jitter_shard(P(o), P(d), SEED, counter, first, batch, S, NEAR, FAR, P(grid), RES, BOUND, P(z), P(slots),
                                                    P(pts), P(dirs), P(count), None) == 0
        torch.cuda.synchronize()
        _REFERENCE[key] = dict(o=o, d=d, target=target, rgba=rgba, z=z, slots=slots, pts=pts, dirs=dirs, count=int(count.item()), grid=grid,
                               counter=counter)
    return _REFERENCE[key]


def outputs(batch, S):
    n = batch * S
    return dict(o=filled(batch, 3), d=filled(batch, 3), rgba=filled(batch, 4), target=filled(batch, 3), z=filled(batch, S),
                slots=filled(n, dtype=torch.int32), pts=filled(n, 3), dirs=filled(n, 3))


def head_args(scene, ref, case, out):
    images, poses, focal, bg = scene
    batch, S, first = CASES[case]
    return (P(images), P(poses), 3, 8, 8, focal, 1.0, P(bg), SEED, ref["counter"], first, batch, S, NEAR, FAR, P(ref["grid"]), RES, BOUND,
            P(out["o"]), P(out["d"]), P(out["rgba"]), P(out["target"]), P(out["z"]), P(out["slots"]), P(out["pts"]), P(out["dirs"]))


def check_against_reference(out, count, ref):
    assert torch.equal(out["o"], ref["o"]) and torch.equal(out["d"], ref["d"])
    assert torch.equal(out["target"], ref["target"]) and torch.equal(out["rgba"], ref["rgba"])
    assert torch.equal(out["z"], ref["z"])
    mine, theirs = out["slots"] >= 0, ref["slots"] >= 0
    assert torch.equal(mine, theirs) and count == ref["count"] == int(mine.sum())
    # the active slots are a permutation of range(count); the rows read through each call's own slot map are the same rows
    assert torch.equal(torch.sort(out["slots"][mine]).values, torch.arange(count, dtype=torch.int32, device="cuda"))
    assert bool((out["slots"][~mine] == -1).all())
    a, b = out["slots"][mine].long(), ref["slots"][theirs].long()
    assert torch.equal(out["pts"][a], ref["pts"][b]) and torch.equal(out["dirs"][a], ref["dirs"][b])
    assert is_filled(out["pts"][count:]) and is_filled(out["dirs"][count:])      # nothing is written from row `count` on


@pytest.mark.parametrize("case,kind", PLAIN_FORM)
def test_plain_form_equals_the_two_calls(ops, lib, scene, case, kind):
    ref = reference(ops, lib, scene, case, kind)
    batch, S, _ = CASES[case]
    out = outputs(batch, S)
    count = filled(1, dtype=torch.int32)                                         # the call clears it
    assert lib.nerf_train_batch_compact(*head_args(scene, ref, case, out), P(count), None) == 0
    torch.cuda.synchronize()
    check_against_reference(out, int(count.item()), ref)
    if kind == "zeros":
        assert int(count.item()) == 0 and bool((out["slots"] == -1).all())
    if kind == "ones" and batch >= 63:
        assert 0 < int(count.item()) < batch * S                                 # rays enter and leave the box: both branches ran


@pytest.mark.parametrize("case", ["one-pass", "several-workgroups-shard"])
def test_rgba_or_target_alone(ops, lib, scene, case):
    ref = reference(ops, lib, scene, case, "seeded")
    batch, S, _ = CASES[case]
    images, poses, focal, bg = scene
    for want in ("rgba", "target"):
        out = outputs(batch, S)
        args = list(head_args(scene, ref, case, out))
        if want == "rgba":
            args[7], args[21] = None, None                                       # bg and target go together
        else:
            args[20] = None
        count = filled(1, dtype=torch.int32)
        assert lib.nerf_train_batch_compact(*args, P(count), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[want], ref[want]) and is_filled(out["target" if want == "rgba" else "rgba"])
        assert int(count.item()) == ref["count"] and torch.equal(out["z"], ref["z"])


def test_chain_form_three_links_and_an_interleaved_compaction(ops, lib, scene):
    """three links on one chain_state: each publishes (count, seq) to its host block, counts in word `turn`, leaves word `turn ^ 1`
    zero; then a link of nerf_sample_compact_jitter_chain and one more link of this entry on the same state"""
    from project_nerf_amd import _lib
    state = torch.zeros(_lib.COMPACT_CHAIN_WORDS, dtype=torch.int32, device="cuda")
    host = torch.zeros(5, 2, dtype=torch.int32).pin_memory()
    plan = [("one-pass", "seeded"), ("several-workgroups-shard", "seeded"), ("4097-second-pass", "ones")]
    turn = 0
    for i, (case, kind) in enumerate(plan):
        ref = reference(ops, lib, scene, case, kind)
        batch, S, _ = CASES[case]
        out = outputs(batch, S)
        assert lib.nerf_train_batch_compact_chain(*head_args(scene, ref, case, out), P(state), turn, host[i].data_ptr(), 100 + i, None) == 0
        torch.cuda.synchronize()
        assert host[i].tolist() == [ref["count"], 100 + i]
        words = state.cpu()
        assert int(words[turn]) == ref["count"] and int(words[turn ^ 1]) == 0 and bool((words[2:] == 0).all())   # tickets back at zero
        check_against_reference(out, int(host[i, 0]), ref)
        turn ^= 1
    # a link of the compaction alone on the same state ...
    ref = reference(ops, lib, scene, "4095-straddle", "seeded")
    batch, S, first = CASES["4095-straddle"]
    n = batch * S
    z, slots, pts, dirs = filled(batch, S), filled(n, dtype=torch.int32), filled(n, 3), filled(n, 3)
    assert lib.nerf_sample_compact_jitter_chain(P(ref["o"]), P(ref["d"]), SEED, ref["counter"], first, batch, S, NEAR, FAR, P(ref["grid"]), RES,
                                                BOUND, P(z), P(slots), P(pts), P(dirs), P(state), turn, host[3].data_ptr(), 103, None) == 0
    torch.cuda.synchronize()
    assert host[3].tolist() == [ref["count"], 103] and int(state[turn ^ 1]) == 0
    turn ^= 1
    # ... and this entry after it still counts from zero
    ref = reference(ops, lib, scene, "several-workgroups-shard", "ones")
    batch, S, _ = CASES["several-workgroups-shard"]
    out = outputs(batch, S)
    assert lib.nerf_train_batch_compact_chain(*head_args(scene, ref, "several-workgroups-shard", out), P(state), turn, host[4].data_ptr(), 104,
                                              None) == 0
    torch.cuda.synchronize()
    assert host[4].tolist() == [ref["count"], 104] and int(state[turn ^ 1]) == 0
    check_against_reference(out, int(host[4, 0]), ref)


def test_ops_entry_shares_the_chain_with_sample_compact_async(ops, lib, scene):
    """ops.train_batch_compact and ops.sample_compact_async alternate on ONE chain per (device, stream): four batches queued ahead
    of any read, every count right"""
    images, poses, focal, bg = scene
    queued = []
    for i, (case, kind) in enumerate([("one-pass", "seeded"), ("4095-straddle", "seeded"), ("several-workgroups-shard", "ones"),
                                      ("4097-second-pass", "seeded")]):
        ref = reference(ops, lib, scene, case, kind)
        batch, S, first = CASES[case]
        if i % 2 == 0:
            o, d, target, prepared = ops.train_batch_compact(images, poses, focal, batch, S, NEAR, FAR, SEED, ref["counter"], ref["grid"], BOUND,
                                                             bg=bg, first_ray=first)
            assert torch.equal(o, ref["o"]) and torch.equal(d, ref["d"]) and torch.equal(target, ref["target"])
        else:
            prepared = ops.sample_compact_async(ref["o"], ref["d"], NEAR, FAR, S, ref["grid"], BOUND, jitter=(SEED, ref["counter"]),
                                                first_ray=first)
        queued.append((prepared, ref))
    chain = ops._COMPACT_CHAIN[(images.device, ops._stream())]
    for prepared, ref in queued:
        z, slots, pts, dirs = prepared.get()
        assert pts.shape[0] == dirs.shape[0] == ref["count"] and torch.equal(z, ref["z"])
        assert torch.equal(slots >= 0, ref["slots"] >= 0)
        a, b = slots[slots >= 0].long(), ref["slots"][ref["slots"] >= 0].long()
        assert torch.equal(pts[a], ref["pts"][b]) and torch.equal(dirs[a], ref["dirs"][b])
    assert ops._COMPACT_CHAIN[(images.device, ops._stream())] is chain
    o, d, rgba, prepared = ops.train_batch_compact(images, poses, focal, 64, 64, NEAR, FAR, SEED, 15, make_grid("seeded"), BOUND, want_rgba=True)
    assert rgba.shape == (64, 4) and torch.equal(rgba, reference(ops, lib, scene, "one-pass", "seeded")["rgba"])
    o, d, target, prepared = ops.train_batch_compact(images, poses, focal, 0, 64, NEAR, FAR, SEED, 15, make_grid("seeded"), BOUND, bg=bg)
    assert o.shape == (0, 3) and prepared.get()[2].shape[0] == 0                  # no rays: no launch of the fused kernel, a count of 0


def test_deterministic_fallback_returns_the_ordered_compaction(ops, lib, scene):
    images, poses, focal, bg = scene
    case = "several-workgroups-shard"
    ref = reference(ops, lib, scene, case, "seeded")
    batch, S, first = CASES[case]
    ops.set_deterministic(True)
    try:
        o, d, target, prepared = ops.train_batch_compact(images, poses, focal, batch, S, NEAR, FAR, SEED, ref["counter"], ref["grid"], BOUND,
                                                         bg=bg, first_ray=first)
        z, slots, pts, dirs = prepared.get()
        z2, slots2, pts2, dirs2 = ops.sample_compact_async(ref["o"], ref["d"], NEAR, FAR, S, ref["grid"], BOUND, jitter=(SEED, ref["counter"]),
                                                           first_ray=first).get()
    finally:
        ops.set_deterministic(False)
    assert torch.equal(o, ref["o"]) and torch.equal(d, ref["d"]) and torch.equal(target, ref["target"])
    assert torch.equal(z, ref["z"]) and torch.equal(slots, slots2) and torch.equal(pts, pts2) and torch.equal(dirs, dirs2)
    active = slots[slots >= 0]
    assert pts.shape[0] == ref["count"] and torch.equal(active, torch.arange(ref["count"], dtype=torch.int32, device="cuda"))   # SAMPLE order
