"""The ray front end against the exact host restatement of tests/frontend_reference.py: pixel draws and ray formation on
frames that are not square, the (seed, counter, global index) -> draw mapping of every kernel that draws, the fused
compaction kernels at the faces of the occupancy grid, the Part 4 coordinate / time noise, the occupancy-grid refresh and
the inverse-CDF resampler.  Everything a kernel computes with individually rounded fp32 operations is compared bit for bit."""
import numpy as np
import pytest
import torch

import frontend_reference as F
from conftest import golden
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

T = torch.from_numpy
P = lambda t: None if t is None else t.data_ptr()
NEAR, FAR = 2.0, 6.0
COUNTER_MAX = 2 ** 24 - 1


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def dev(a):
    if isinstance(a, np.ndarray):
        a = T(np.ascontiguousarray(a))
    return a.cuda()


def synth_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * 4.0311
    d = (torch.rand(n, 3, generator=g) - 0.5) * 1.6 - o
    return o, d / d.norm(dim=-1, keepdim=True)


# =================================================================================================== batch kernels
_SCENES = {}


def scene(name):
    """frames [n,H,W,4] with H != W, random orthonormal poses, focal, scene scale, background -- host and device copies"""
    if name not in _SCENES:
        n, H, W, focal, scale = {"3x5x7": (3, 5, 7, 6.25, 1.0), "2x9x4": (2, 9, 4, 5.5, 0.5)}[name]
        rng = np.random.default_rng(n * 100 + H * 10 + W)
        frames = rng.random((n, H, W, 4), dtype=np.float32)
        poses = F.random_poses(n, rng)
        bg = np.array([0.3, 0.6, 0.9], dtype=np.float32)
        _SCENES[name] = dict(frames=frames, poses=poses, focal=focal, scale=scale, bg=bg, frames_gpu=dev(frames), poses_gpu=dev(poses),
                             bg_gpu=dev(bg))
    return _SCENES[name]


def run_train_batch(ops, sc, batch, S, seed, counter, first_ray, perturb, with_bg=True):
    return ops.train_batch(sc["frames_gpu"], sc["poses_gpu"], sc["focal"], batch, S, NEAR, FAR, seed, counter,
                           bg=sc["bg_gpu"] if with_bg else None, scene_scale=sc["scale"], perturb=perturb, first_ray=first_ray)


def check_train_batch(ops, sc, batch, S, seed, counter, first_ray, perturb):
    ref = F.train_batch_reference(sc["frames"], sc["poses"], sc["focal"], sc["scale"], sc["bg"], seed, counter, first_ray, batch, S,
                                  NEAR, FAR, perturb)
    o, d, target, z = run_train_batch(ops, sc, batch, S, seed, counter, first_ray, perturb)
    o2, d2, rgba, z2 = run_train_batch(ops, sc, batch, S, seed, counter, first_ray, perturb, with_bg=False)
    assert torch.equal(o.cpu(), T(ref["o"])) and torch.equal(o2, o)
    assert torch.equal(rgba.cpu(), T(ref["rgba"]))
    assert torch.equal(target.cpu(), T(ref["target"]))
    assert torch.equal(z.cpu(), ref["z"]) and torch.equal(z2, z)
    assert float((d.cpu() - T(ref["d"])).abs().max()) <= 3e-7 and torch.equal(d2, d)
    return o, d, target, z


@pytest.mark.parametrize("perturb", [True, False], ids=["jitter", "plain"])
@pytest.mark.parametrize("batch,S", [(4099, 5), (257, 64)])
@pytest.mark.parametrize("name", ["3x5x7", "2x9x4"])
def test_train_batch_equals_the_host_reference(ops, name, batch, S, perturb):
    sc = scene(name)
    whole = check_train_batch(ops, sc, batch, S, 7, 5, 0, perturb)
    # the batch split at first_ray: the tail, drawn on its own, is the tail of the whole
    for first in (1, 1000, 4098):
        if first < batch:
            part = run_train_batch(ops, sc, batch - first, S, 7, 5, first, perturb)
            for got, want in zip(part, whole):
                assert torch.equal(got, want[first:])
        check_train_batch(ops, sc, min(batch, 300), S, 7, 5, first, perturb)       # and a shard that starts there, against the host


def test_train_batch_at_its_limits(ops):
    sc = scene("3x5x7")
    lib_error = ops._lib.NerfHipError
    check_train_batch(ops, sc, 257, 5, 11, COUNTER_MAX, 3, True)
    with pytest.raises(lib_error):
        run_train_batch(ops, sc, 257, 5, 11, COUNTER_MAX + 1, 3, True)
    batch, S = 3, 5
    first = (2 ** 39 - 1) // S - batch                              # (first + batch) * S <= 2^39 - 1
    assert (first + batch) * S < 2 ** 39 <= (first + 1 + batch) * S
    check_train_batch(ops, sc, batch, S, 11, COUNTER_MAX, first, True)
    with pytest.raises(lib_error):
        run_train_batch(ops, sc, batch, S, 11, COUNTER_MAX, first + 1, True)


@pytest.mark.parametrize("name", ["3x5x7", "2x9x4"])
def test_gather_kernels_on_frames_that_are_not_square(ops, name):
    sc = scene(name)
    n, H, W, _ = sc["frames"].shape
    rng = np.random.default_rng(8)
    flat = np.concatenate([[0, n * H * W - 1, W - 1, W, H * W - 1, H * W], rng.integers(0, n * H * W, 1000)]).astype(np.int64)
    im, py, px = F.pixel_of(flat, H, W)
    o_ref, d_ref = F.rays_of_pixels(sc["poses"], im, py, px, H, W, sc["focal"], sc["scale"])
    rgba_ref = sc["frames"][im, py, px]
    o, d, target, rgba = ops.gather_batch(sc["frames_gpu"], sc["poses_gpu"], dev(flat), sc["focal"], sc["scale"], bg=sc["bg_gpu"], want_rgba=True)
    assert torch.equal(o.cpu(), T(o_ref)) and torch.equal(rgba.cpu(), T(rgba_ref))
    assert torch.equal(target.cpu(), T(F.composite_target(rgba_ref, sc["bg"])))
    assert float((d.cpu() - T(d_ref)).abs().max()) <= 3e-7
    o3, d3, rgba3 = ops.gather_rays(sc["frames_gpu"], sc["poses_gpu"], dev(im), dev(py), dev(px), sc["focal"], sc["scale"])
    assert torch.equal(o3, o) and torch.equal(d3, d) and torch.equal(rgba3, rgba)


# =================================================================================================== compaction
FORMS = ["single_pass", "ordered"]


def run_compact(ops, form, o, d, S, bits, bound, u=None, jitter=None, first_ray=0):
    """nerf_sample_compact / _jitter_shard (single pass) or nerf_sample_compact_ordered through the C ABI, outputs pre-filled:
    (z, slots, pts[:n], dirs[:n], n)"""
    lib = ops._lib.load()
    R, n = o.shape[0], o.shape[0] * S
    z = torch.full((R, S), -7.0, device="cuda")
    slots = torch.full((n,), -7, device="cuda", dtype=torch.int32)
    pts, dirs = torch.full((max(n, 1), 3), -7.0, device="cuda"), torch.full((max(n, 1), 3), -7.0, device="cuda")
    count = torch.full((1,), 12345, device="cuda", dtype=torch.int32)
    seed, counter = jitter if jitter is not None else (0, 0)
    res, st = bits.shape[0], ops._stream()
    if form == "ordered":
        scratch = torch.empty(max(lib.nerf_sample_compact_ordered_scratch_bytes(R, S), 4), dtype=torch.uint8, device="cuda")
        code = lib.nerf_sample_compact_ordered(P(o), P(d), P(u), 1 if jitter is not None else 0, seed, counter, first_ray, R, S, NEAR, FAR,
                                               P(bits), res, bound, P(z), P(slots), P(pts), P(dirs), P(count), P(scratch), scratch.numel(), st)
    elif jitter is not None:
        code = lib.nerf_sample_compact_jitter_shard(P(o), P(d), seed, counter, first_ray, R, S, NEAR, FAR, P(bits), res, bound, P(z), P(slots),
                                                    P(pts), P(dirs), P(count), st)
    else:
        code = lib.nerf_sample_compact(P(o), P(d), P(u), R, S, NEAR, FAR, P(bits), res, bound, P(z), P(slots), P(pts), P(dirs), P(count), st)
    ops._lib.check(code, f"compaction ({form})")
    n_act = int(count.item())
    assert 0 <= n_act <= n
    return z, slots, pts[:n_act], dirs[:n_act], n_act


def check_compaction(form, out, o, d, z_ref, bits, bound, compare_dirs=True):
    """depths bit for bit; slots, points and count against the oracle's occupancy test of the points of those depths"""
    z, slots, pts_c, dirs_c, n_act = out
    assert torch.equal(z.cpu(), z_ref)
    pts_ref, dirs_ref = O.ray_points(o, d, z_ref)
    mask = O.active_mask(pts_ref, bits, bound)
    slots = slots.cpu()
    assert torch.equal(slots >= 0, mask)
    assert bool((slots[~mask] == -1).all())
    assert n_act == int(mask.sum()) == pts_c.shape[0]
    act = slots[mask].long()
    if form == "ordered":
        assert torch.equal(act, torch.arange(n_act))                            # slots in sample order
    else:
        assert torch.equal(torch.sort(act).values, torch.arange(n_act))         # a permutation
    assert torch.equal(pts_c.cpu()[act], pts_ref[mask])
    if compare_dirs and n_act:
        np.testing.assert_allclose(dirs_c.cpu()[act].numpy(), dirs_ref[mask].numpy(), rtol=2e-7)
    return mask


_BITS = {}


def random_bits(res, p, seed):
    if (res, p, seed) not in _BITS:
        b = torch.rand(res, res, res, generator=torch.Generator().manual_seed(seed)) < p
        _BITS[(res, p, seed)] = (b, b.cuda())
    return _BITS[(res, p, seed)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("R,S,first_ray,counter", [(R, S, f, c) for R, S in ((77, 64), (3, 5)) for f in (0, 100) for c in (0, COUNTER_MAX)]
                         + [(3, 5, (2 ** 40 - 1) // 5 - 3, 9)])
def test_compaction_jitter_is_the_host_draw_at_the_global_index(ops, form, R, S, first_ray, counter):
    seed = 21
    o, d = synth_rays(R, 23)
    bits, bits_gpu = random_bits(128, 0.2, 3)
    assert (first_ray + R) * S < 2 ** 40
    u = F.jitter_uniforms(counter, first_ray, R, S, F.squares_key(seed))
    z_ref = O.stratified_depths(NEAR, FAR, S, R, True, u=T(u)).contiguous()
    out = run_compact(ops, form, dev(o), dev(d), S, bits_gpu, 1.5, jitter=(seed, counter), first_ray=first_ray)
    mask = check_compaction(form, out, o, d, z_ref, bits, 1.5)
    assert R * S < 100 or 0 < int(mask.sum()) < R * S


@pytest.mark.parametrize("form", FORMS)
def test_compaction_jitter_refuses_what_its_stream_cannot_hold(ops, form):
    o, d = synth_rays(3, 23)
    _, bits_gpu = random_bits(128, 0.2, 3)
    first = (2 ** 40 - 1) // 5 - 3
    with pytest.raises(ops._lib.NerfHipError):
        run_compact(ops, form, dev(o), dev(d), 5, bits_gpu, 1.5, jitter=(21, 9), first_ray=first + 1)
    with pytest.raises(ops._lib.NerfHipError):
        run_compact(ops, form, dev(o), dev(d), 5, bits_gpu, 1.5, jitter=(21, COUNTER_MAX + 1), first_ray=0)


def edge_points(res, bound):
    """the eight edge points of golden g3 (bound 1.5) and, on every axis, the values one ulp either side of +bound, -bound and
    -bound - 1/scale (where the scaled coordinate crosses -1: truncation toward zero still gives voxel 0 above it)"""
    f32 = np.float32
    pts = [golden(f"g3_mask_res{res}")["pts"][:8].astype(f32)]
    scale = f32(res / (2.0 * bound))
    for c in (f32(bound), f32(-bound), f32(-bound) - f32(1.0) / scale):
        for v in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
            for axis in range(3):
                p = np.full(3, 0.1, dtype=f32)
                p[axis] = v
                pts.append(p[None])
    return np.concatenate(pts, 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("res", [64, 128])
def test_compaction_at_the_faces_of_the_grid(ops, form, res):
    """rays that do not move (rays_d = 0): every sample sits exactly on the ray's origin"""
    S, bound = 5, 1.5
    pts = edge_points(res, bound)
    o, d = T(pts), torch.zeros(pts.shape[0], 3)
    z_ref = O.stratified_depths(NEAR, FAR, S, pts.shape[0], False).contiguous()
    assert torch.equal(O.ray_points(o, d, z_ref)[0], o.repeat_interleave(S, 0))
    masks = []
    for bits in (T(golden(f"g3_mask_res{res}")["bits"]), torch.ones(res, res, res, dtype=torch.bool)):
        out = run_compact(ops, form, dev(o), dev(d), S, bits.cuda(), bound)
        masks.append(check_compaction(form, out, o, d, z_ref, bits, bound, compare_dirs=False))     # directions are 0 / 0 here
    inside = masks[1].view(-1, S)[:, 0]
    assert 0 < int(inside.sum()) < inside.numel()
    # the band (-1, 0) of the scaled coordinate belongs to voxel 0, the value -1 itself does not
    scaled = (T(pts) + bound) * (res / (2 * bound))
    band = ((scaled > -1) & (scaled < 0)).any(-1)
    assert int(band.sum()) >= 3 and bool(inside[band & (scaled < res).all(-1) & (scaled > -1).all(-1)].all())


@pytest.mark.parametrize("form", FORMS)
def test_compaction_with_nothing_and_with_everything_set(ops, form):
    R, S, res, bound = 37, 17, 32, 1.5
    o, d = synth_rays(R, 31)
    u = torch.rand(R, S, generator=torch.Generator().manual_seed(2))
    z_ref = O.stratified_depths(NEAR, FAR, S, R, True, u=u).contiguous()
    empty = torch.zeros(res, res, res, dtype=torch.bool)
    z, slots, pts_c, dirs_c, n_act = out = run_compact(ops, form, dev(o), dev(d), S, empty.cuda(), bound, u=dev(u))
    check_compaction(form, out, o, d, z_ref, empty, bound)
    assert n_act == 0 and pts_c.shape == (0, 3) and dirs_c.shape == (0, 3) and bool((slots == -1).all())
    # compositing through that map: no row of the field's outputs is referenced (one row of poison stands in for them)
    bg = dev(torch.tensor([0.3, 0.6, 0.9]))
    c, dep, acc = ops.composite_indexed(torch.full((1, 3), 1e9, device="cuda"), torch.full((1,), 1e9, device="cuda"), slots, z, dev(d), bg)
    assert torch.equal(c, bg.expand(R, 3)) and bool((acc == 0).all()) and bool((dep == 0).all())
    full = torch.ones(res, res, res, dtype=torch.bool)
    out = run_compact(ops, form, dev(o), dev(d), S, full.cuda(), bound, u=dev(u))
    mask = check_compaction(form, out, o, d, z_ref, full, bound)
    assert 0 < int(mask.sum()) < R * S                             # the rays enter and leave the box


@pytest.mark.parametrize("form", FORMS)
def test_compaction_with_a_scale_that_is_no_power_of_two(ops, form):
    R, S, res, bound = 200, 64, 100, 1.3
    o, d = synth_rays(R, 41)
    bits, bits_gpu = random_bits(res, 0.3, 6)
    u = torch.rand(R, S, generator=torch.Generator().manual_seed(4))
    z_ref = O.stratified_depths(NEAR, FAR, S, R, True, u=u).contiguous()
    out = run_compact(ops, form, dev(o), dev(d), S, bits_gpu, bound, u=dev(u))
    mask = check_compaction(form, out, o, d, z_ref, bits, bound)
    assert 0 < int(mask.sum()) < R * S


# =================================================================================================== Part 4 noise
# Largest |kernel - fp64 reference| of a normal, recovered as (x' - x) / std_x or (t' - t) / std_t: MEASURED_NOISE_ERROR on an
# MI355X (v_sin_f32 and the fast logarithm carry no quotable bound; 9.9e-7 on the slot-mapped cases, 1.375e-6 in point mode;
# up to 4.8e-7 of it is the fp32 rounding of x' seen through 1 / std_x).  The tests assert four times the largest, rounded up to one
# digit.  A wrong index gives differences of order 1; a measurement above 1e-3 would mean a wrong kernel, not a wider bound.
MEASURED_NOISE_ERROR = 1.375e-6
NOISE_TOL = 6e-6
SENTINEL = -1234.5


def p4_inputs(ops, slots, pts, times, n_rays, n_samples, std_x, std_t, seed, counter, first_ray, x_out, t_out):
    lib = ops._lib.load()
    ops._lib.check(lib.nerf_p4_sample_inputs(P(slots), P(pts), P(times), n_rays, n_samples, float(std_x), float(std_t), seed, counter, first_ray,
                                             P(x_out), P(t_out), ops._stream()), "nerf_p4_sample_inputs")


def p4_case(R=41, S=17):
    """a slot map that is a random permutation with holes into compact arrays with a few rows nobody points at"""
    rng = np.random.default_rng(17)
    n = R * S
    active = rng.random(n) < 0.6
    n_act = int(active.sum())
    rows = n_act + 5
    slots = np.full(n, -1, dtype=np.int32)
    slots[active] = rng.permutation(rows)[:n_act].astype(np.int32)
    pts = (rng.random((rows, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    times = rng.random(R, dtype=np.float32)
    times[::5], times[1::5] = 0.0, 1.0                               # both clamps of t' fire
    return dict(R=R, S=S, slots=slots, active=active, rows=rows, pts=pts, times=times,
                used=np.isin(np.arange(rows), slots[active]))


def test_p4_inputs_without_noise_pass_the_times_through(ops):
    from project_nerf_amd import dynamic_engine as DE
    c = p4_case()
    R, S, rows = c["R"], c["S"], c["rows"]
    slots, pts, times = dev(c["slots"]), dev(c["pts"]), dev(c["times"])
    x_out, t_out = torch.full((rows, 3), SENTINEL, device="cuda"), torch.full((rows,), SENTINEL, device="cuda")
    p4_inputs(ops, slots, pts, times, R, S, 0.0, 0.0, 5, 3, 0, x_out, t_out)
    want_t = np.full(rows, SENTINEL, dtype=np.float32)
    want_t[c["slots"][c["active"]]] = np.repeat(c["times"], S)[c["active"]]
    want_x = np.where(c["used"][:, None], c["pts"], np.float32(SENTINEL))
    assert torch.equal(t_out.cpu(), T(want_t)) and torch.equal(x_out.cpu(), T(want_x))
    x_def, t_def = DE.sample_inputs(slots, pts, times.view(R, 1), R, S)          # the wrapper: no x' without coordinate noise
    assert x_def is None and torch.equal(t_def.cpu()[c["used"]], T(want_t)[c["used"]])
    # point mode: one time per point, no slot map
    t_pts = dev(np.random.default_rng(3).random(rows, dtype=np.float32))
    x_def, t_def = DE.sample_inputs(None, pts, t_pts, rows, 0)
    assert x_def is None and torch.equal(t_def, t_pts)


@pytest.mark.parametrize("first_ray", [0, 37, (2 ** 38 - 1) // 17 - 41])
def test_p4_noise_is_the_host_normal_at_the_global_sample(ops, first_ray):
    c = p4_case()
    R, S, rows = c["R"], c["S"], c["rows"]
    assert (first_ray + R) * S < 2 ** 38
    seed, counter, std_x, std_t = 5, 3, 0.25, 0.5
    slots, pts, times = dev(c["slots"]), dev(c["pts"]), dev(c["times"])
    x_out, t_out = torch.full((rows, 3), SENTINEL, device="cuda"), torch.full((rows,), SENTINEL, device="cuda")
    p4_inputs(ops, slots, pts, times, R, S, std_x, std_t, seed, counter, first_ray, x_out, t_out)
    x, t = x_out.cpu().numpy().astype(np.float64), t_out.cpu().numpy().astype(np.float64)
    assert (x[~c["used"]] == SENTINEL).all() and (t[~c["used"]] == SENTINEL).all()        # rows nobody points at: untouched
    g = np.nonzero(c["active"])[0]
    row = c["slots"][g]
    normal = F.normal_noise(counter, first_ray * S + g, F.noise_key(seed))
    err_x = np.abs((x[row] - c["pts"][row].astype(np.float64)) / std_x - normal[:, :3])
    t_ray = c["times"][g // S].astype(np.float64)
    raw = t_ray + normal[:, 3] * std_t
    free = (raw > 1e-3) & (raw < 1 - 1e-3)
    err_t = np.abs((t[row][free] - t_ray[free]) / std_t - normal[free, 3])
    print(f"[noise] first_ray {first_ray}: max |kernel - fp64| = {max(err_x.max(), err_t.max()):.3e} (x {err_x.max():.3e}, t {err_t.max():.3e})")
    assert err_x.max() <= NOISE_TOL and err_t.max() <= NOISE_TOL
    assert (t[row][raw < -1e-3] == 0.0).all() and (t[row][raw > 1 + 1e-3] == 1.0).all()
    assert (raw < -1e-3).sum() > 10 and (raw > 1 + 1e-3).sum() > 10 and free.sum() > 100
    assert t[row].min() >= 0.0 and t[row].max() <= 1.0
    # two shards of the rays equal the whole, bit for bit
    x2, t2 = torch.full((rows, 3), SENTINEL, device="cuda"), torch.full((rows,), SENTINEL, device="cuda")
    for a, b in ((0, 20), (20, R)):
        p4_inputs(ops, slots[a * S:b * S], pts, times[a:b], b - a, S, std_x, std_t, seed, counter, first_ray + a, x2, t2)
    assert torch.equal(x2, x_out) and torch.equal(t2, t_out)
    # only the time noise: no x' is written, t' is the same
    t3 = torch.full((rows,), SENTINEL, device="cuda")
    p4_inputs(ops, slots, pts, times, R, S, 0.0, std_t, seed, counter, first_ray, None, t3)
    assert torch.equal(t3, t_out)


def test_p4_noise_in_point_mode(ops):
    n, first = 1000, 37
    rng = np.random.default_rng(9)
    pts, times = rng.random((n, 3), dtype=np.float32), (0.25 + 0.5 * rng.random(n, dtype=np.float32)).astype(np.float32)
    x_out, t_out = torch.full((n, 3), SENTINEL, device="cuda"), torch.full((n,), SENTINEL, device="cuda")
    p4_inputs(ops, None, dev(pts), dev(times), n, 0, 0.25, 0.125, 5, COUNTER_MAX, first, x_out, t_out)
    normal = F.normal_noise(COUNTER_MAX, first + np.arange(n), F.noise_key(5))
    err_x = np.abs((x_out.cpu().numpy().astype(np.float64) - pts) / 0.25 - normal[:, :3]).max()
    raw = times + normal[:, 3] * 0.125
    free = (raw > 1e-3) & (raw < 1 - 1e-3)
    err_t = np.abs((t_out.cpu().numpy().astype(np.float64) - times) / 0.125 - normal[:, 3])[free].max()
    print(f"[noise] point mode: max |kernel - fp64| = {max(err_x, err_t):.3e}")
    assert err_x <= NOISE_TOL and err_t <= NOISE_TOL and free.sum() > 900


def test_p4_inputs_refuse_samples_whose_draws_leave_the_stream(ops):
    c = p4_case()
    R, S, rows = c["R"], c["S"], c["rows"]
    slots, pts, times = dev(c["slots"]), dev(c["pts"]), dev(c["times"])
    x_out, t_out = torch.empty(rows, 3, device="cuda"), torch.empty(rows, device="cuda")
    first = (2 ** 38 - 1) // S - R                                   # the last admissible first_ray (used above)
    assert (first + R) * S < 2 ** 38 <= (first + 1 + R) * S
    err = ops._lib.NerfHipError
    with pytest.raises(err):
        p4_inputs(ops, slots, pts, times, R, S, 0.25, 0.5, 5, 3, first + 1, x_out, t_out)
    with pytest.raises(err):
        p4_inputs(ops, slots, pts, times, R, S, 0.25, 0.5, 5, 3, 2 ** 62, x_out, t_out)
    with pytest.raises(err):
        p4_inputs(ops, None, pts, dev(np.zeros(rows, dtype=np.float32)), rows, 0, 0.25, 0.5, 5, 3, 2 ** 38 - rows, x_out, t_out)
    with pytest.raises(err):
        p4_inputs(ops, slots, pts, times, R, S, 0.25, 0.5, 5, COUNTER_MAX + 1, 0, x_out, t_out)
    p4_inputs(ops, None, pts, dev(np.zeros(rows, dtype=np.float32)), rows, 0, 0.25, 0.5, 5, 3, 2 ** 38 - rows - 1, x_out, t_out)


# =================================================================================================== grid refresh
@pytest.mark.parametrize("bound", [1.5, 1.3])
@pytest.mark.parametrize("res", [2, 3, 33, 128])
def test_grid_lattice_equals_linspace_meshgrid(ops, res, bound):
    got = ops.grid_lattice(bound, res, "cuda")                       # 128^3 cells: four trips of the 2048 x 256 launch
    assert torch.equal(got.cpu(), O.grid_lattice(bound, res))


THRESHOLD = float(np.float32(0.01))


@pytest.mark.parametrize("mode", ["static", "dynamic_1.0", "dynamic_0.95"])
@pytest.mark.parametrize("n", [1, 63, 65, 2048 * 256 + 77, 128 ** 3])
def test_grid_threshold_equals_torch(ops, n, mode):
    f32 = np.float32
    rng = np.random.default_rng(n % 1000)
    thr = f32(THRESHOLD)
    cur = (rng.random(n, dtype=f32) * f32(0.02)).astype(f32)
    prev = (rng.random(n, dtype=f32) * f32(0.02)).astype(f32)
    decay = f32(1.0 if mode != "dynamic_0.95" else 0.95)
    up, down = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    if n >= 63:
        k = np.arange(0, n, max(n // 40, 1))[:36].reshape(4, 9)       # spread over the array, last rows included
        k[3] = n - 1 - np.arange(9)
        # at the threshold, one ulp above, one ulp below (the running maximum must not lift them: prev = 0)
        cur[k[0, 0:3]], cur[k[0, 3:6]], cur[k[0, 6:9]] = thr, up(thr), down(thr)
        prev[k[0]] = 0.0
        # prev * decay ties with sigma, or sits one ulp to either side of it
        tie = (prev[k[1]] * decay).astype(f32)
        cur[k[1, 0:3]], cur[k[1, 3:6]], cur[k[1, 6:9]] = tie[0:3], up(tie[3:6]), down(tie[6:9])
        # the decayed previous value alone decides, exactly at / around the threshold
        for j, target in ((0, thr), (1, up(thr)), (2, down(thr))):
            idx = k[2, 3 * j:3 * j + 3]
            prev[idx] = target if decay == 1.0 else (f32(target) / decay).astype(f32)
            cur[idx] = 0.0
        cur[k[3, 0:3]], cur[k[3, 3:6]], cur[k[3, 6:9]] = thr, up(thr), down(thr)
        prev[k[3]] = 0.0
    else:
        cur[0] = thr
    dynamic = mode != "static"
    cur_t, prev_t = T(cur), T(prev)
    grid_ref = torch.maximum(prev_t * torch.tensor(decay), cur_t) if dynamic else cur_t
    bin_ref = grid_ref > torch.tensor(thr)
    count_ref = int(bin_ref.sum())
    cur_g, prev_g = dev(cur), dev(prev)
    binary, ratio = ops.grid_threshold(cur_g, THRESHOLD, prev=prev_g if dynamic else None, decay=float(decay))
    assert torch.equal((prev_g if dynamic else cur_g).cpu(), grid_ref)
    assert torch.equal(binary.cpu(), bin_ref)
    assert ratio == float(count_ref) / n
    assert n < 63 or 0 < count_ref < n


# =================================================================================================== inverse-CDF resampler
def check_sample_pdf(ops, S, NF, R):
    z, w, u = F.pdf_case(S, NF, R)
    out = ops.sample_pdf(dev(z), dev(w), NF, dev(u)).cpu().numpy()
    assert out.shape == (R, S + NF) and np.isfinite(out).all()
    assert (out[:, 1:] >= out[:, :-1]).all()
    z, w, u = z.numpy(), w.numpy(), u.numpy()
    fine = F.fine_of_merged(out, z)                                  # every coarse depth is there bit for bit, NF values remain
    assert fine is not None and fine.shape == (R, NF)
    tol, mass = F.pdf_tolerance(z, w, u)
    heavy = float((mass > 100.0 * tol).mean())
    assert heavy >= 0.85                                             # (on the reference alone) a slip of one bin would fail
    ratio = np.abs(F.pdf_forward_cdf(z, w, fine) - u) / tol
    print(f"[pdf {S}x{NF}, {R} rays] error / tolerance {ratio.max():.3f}, draws in bins heavier than 100 tol: {heavy:.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("S,NF", F.PDF_SHAPES)
def test_sample_pdf_inverts_the_cdf(ops, S, NF):
    check_sample_pdf(ops, S, NF, F.PDF_RAYS)


def test_sample_pdf_strides_over_more_rays_than_workgroups(ops):
    check_sample_pdf(ops, 3, 2, 65536 + 3)


@pytest.mark.parametrize("NF", [1, 2, 5, 128, 129])
def test_sample_pdf_default_draws_are_linspace(ops, NF):
    z, w, _ = F.pdf_case(64, NF)
    u = torch.linspace(0.0, 1.0, NF).expand(F.PDF_RAYS, NF).contiguous()
    assert NF > 1 or float(u[0, 0]) == 0.0
    got = ops.sample_pdf(dev(z), dev(w), NF, None)
    want = ops.sample_pdf(dev(z), dev(w), NF, dev(u))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
