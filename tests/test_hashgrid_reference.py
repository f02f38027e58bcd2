"""The fp64 corner-list reference of the hash grid (tests/hashgrid_reference.py) against the oracle, before the GPU
tests rest on it: exact indices, features and both gradients against autograd of oracle.hash_encode with a float64 table, the
closed clamp interval, the sensitivity of the probe set to three typical mistakes, and the operand-image decoder
against an independent encoder."""
import numpy as np
import pytest
import torch

import hashgrid_reference as H
from oracle import nerf_oracle as O

TABLES = list(H.LEVEL_TABLES)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (n_levels, log2_t, base, pls, bound) in H.LEVEL_TABLES.items():
        levels = O.hash_grid_levels(n_levels, log2_t, base, pls)
        pts = H.probe_points(levels, bound, seed=0)
        rng = np.random.default_rng(11)
        table = rng.standard_normal((O.hash_grid_entries(levels), 2))
        d_feat = rng.standard_normal((pts.shape[0], 2 * n_levels))
        d_feat[::7] = 0.0
        out[name] = dict(levels=levels, bound=bound, pts=pts, table=table, d_feat=d_feat, ref=H.HashReference(pts, levels, bound))
    return out


def oracle_autograd(case, table):
    """oracle.hash_encode with a float64 table at the fp32 positions.  The oracle keeps its weights in an fp32 tensor
    whatever the dtype of x01, so it cannot be driven in float64 without editing it: positions, cells and weights are
    its own fp32 ones (the cells therefore the build's), the blend and both gradients' sums run in float64, and the
    comparison is at the fp32 bounds -- of which only the weights' roundings are in play here."""
    x = torch.from_numpy(case["pts"]).requires_grad_(True)
    feat = O.hash_encode(case["levels"], table, O.hash_normalise(x, case["bound"]))
    assert feat.dtype == torch.float64
    return x, feat


@pytest.mark.parametrize("name", TABLES)
def test_indices_equal_the_oracle(cases, name):
    c = cases[name]
    ref_idx, ref_w = O.hash_grid_index(c["levels"], O.hash_normalise(torch.from_numpy(c["pts"]), c["bound"]))
    assert np.array_equal(c["ref"].idx, ref_idx.numpy())
    # the oracle's fp32 weights: three roundings away from the float64 products
    assert np.all(np.abs(c["ref"].w - ref_w.numpy().astype(np.float64)) <= 3 * H.U * c["ref"].w)
    # the level tables are the ones the issue names: every dense level of the small-res table wraps at its upper faces
    if name == "dense_small_res":
        assert [lv.res for lv in c["levels"]] == [4, 6, 9] and [lv.size for lv in c["levels"]] == [64, 216, 736]
        assert all(lv.dense for lv in c["levels"])
    if name == "nodes_l4_t14":
        lv = c["levels"]
        assert lv[0].scale == 16.0 and lv[0].size == 4920 and lv[0].dense and not lv[1].dense
        assert bool((c["ref"].frac[:, 0] == 0.0).all(axis=-1).sum() >= 16)          # the exact-node probes


@pytest.mark.parametrize("name", TABLES)
def test_features_and_gradients_equal_autograd_of_the_oracle(cases, name):
    c = cases[name]
    ref = c["ref"]
    table = torch.from_numpy(c["table"]).requires_grad_(True)
    x, feat = oracle_autograd(c, table)
    mine = ref.features(c["table"])
    # three roundings per fp32 weight (forward_bound's count); the products and sums are float64 on both sides
    assert np.all(np.abs(mine - feat.detach().numpy()) <= 3 * H.U * ref.abs_terms + 1e-12 * ref.abs_terms)
    assert np.all(np.abs(mine - feat.detach().numpy()) <= H.forward_bound(ref.abs_terms))
    g_table, g_x = torch.autograd.grad((feat * torch.from_numpy(c["d_feat"])).sum(), [table, x])
    grad, count, abs_sum = ref.table_gradient(c["d_feat"])
    assert np.all(np.abs(grad - g_table.numpy()) <= (3 * H.U + 1e-12) * abs_sum)
    assert np.all(np.abs(grad - g_table.numpy()) <= H.scatter_float_bound(count, abs_sum, ref.n))
    assert np.array_equal(count == 0, abs_sum.sum(axis=1) == 0.0) or bool((ref.w == 0.0).any())
    d_pts = ref.input_gradient(c["table"], c["d_feat"])
    # fp32 autograd through the oracle's weights, frac, pos and the clamp: the fp32 bound of the kernel's own path
    assert np.all(np.abs(d_pts - g_x.numpy().astype(np.float64)) <= H.input_gradient_bound(ref.abs_input_terms, len(c["levels"])))
    assert np.array_equal(g_x.numpy() == 0.0, d_pts == 0.0)              # the same axes are cut by the clamp
    assert float(np.abs(d_pts).max()) > 0.0


@pytest.mark.parametrize("name", TABLES)
def test_clamp_interval_is_closed(cases, name):
    """exactly +-bound: the gradient passes (the reference and torch.clamp's autograd agree, see above; here: it is not
    zero); strictly outside in this build's fp32 x01: exactly 0.  One ulp outside -bound is outside; one ulp outside
    +bound is NOT: x + bound rounds (ties to even) to 2 bound, x01 == 1 -- the first float outside is two ulps away."""
    c = cases[name]
    b = np.float32(c["bound"])
    inf = np.float32(np.inf)
    d_feat = np.ones((1, 2 * len(c["levels"])))

    def grad_at(v, axis):
        p = (np.asarray([[0.31, -0.17, 0.077]], dtype=np.float32) * b)
        p[0, axis] = v
        return H.HashReference(p, c["levels"], c["bound"]).input_gradient(c["table"], d_feat)[0]
    for axis in range(3):
        assert grad_at(b, axis)[axis] != 0.0 and grad_at(-b, axis)[axis] != 0.0
        assert grad_at(np.nextafter(b, -inf), axis)[axis] != 0.0 and grad_at(np.nextafter(-b, inf), axis)[axis] != 0.0
        out = grad_at(np.nextafter(-b, -inf), axis)
        assert out[axis] == 0.0 and np.all(np.delete(out, axis) != 0.0)
        assert grad_at(np.nextafter(np.nextafter(b, inf), inf), axis)[axis] == 0.0
        assert grad_at(np.float32(10.0) * b, axis)[axis] == 0.0 and grad_at(np.float32(-10.0) * b, axis)[axis] == 0.0
        one_out = np.nextafter(b, inf)
        assert H.normalise_f32(np.asarray([[one_out] * 3]), c["bound"])[0, 0] == np.float32(1.0)
        assert grad_at(one_out, axis)[axis] == grad_at(b, axis)[axis] != 0.0
    # the probe set holds all of these
    raw = H.normalise_f32(c["pts"], c["bound"])
    assert (raw == 1.0).any() and (raw == 0.0).any() and (raw > 1.0).any() and (raw < 0.0).any()


@pytest.mark.parametrize("name", TABLES)
def test_probe_set_sees_typical_mistakes(cases, name):
    """swapped axis weights, a flipped corner sign and an open clamp interval each move the reference by more than the
    bound the GPU tests allow, somewhere on the probe set"""
    c = cases[name]
    ref, L = c["ref"], len(c["levels"])
    feat = ref.features(c["table"])
    fwd_bound = H.forward_bound(ref.abs_terms)
    grad, count, abs_sum = ref.table_gradient(c["d_feat"])
    amax = float(np.abs(c["d_feat"]).max())
    table_bound = np.maximum(H.scatter_float_bound(count, abs_sum, ref.n), H.scatter_fixed_bound(count, abs_sum, amax, ref.n))
    d_pts = ref.input_gradient(c["table"], c["d_feat"])
    in_bound = H.input_gradient_bound(ref.abs_input_terms, L)

    swapped = H.HashReference(c["pts"], c["levels"], c["bound"], mutate="swap_axis_weights")
    assert np.array_equal(swapped.idx, ref.idx)
    assert H.worst_fraction(np.abs(swapped.features(c["table"]) - feat), fwd_bound) > 1e3
    assert H.worst_fraction(np.abs(swapped.table_gradient(c["d_feat"])[0] - grad), table_bound) > 1e3
    assert H.worst_fraction(np.abs(swapped.input_gradient(c["table"], c["d_feat"]) - d_pts), in_bound) > 1e3
    flipped = H.HashReference(c["pts"], c["levels"], c["bound"], mutate="flip_corner_sign")
    assert H.worst_fraction(np.abs(flipped.input_gradient(c["table"], c["d_feat"]) - d_pts), in_bound) > 1e3
    opened = H.HashReference(c["pts"], c["levels"], c["bound"], mutate="open_clamp")
    diff = np.abs(opened.input_gradient(c["table"], c["d_feat"]) - d_pts)
    assert H.worst_fraction(diff, in_bound) > 1e3
    raw = H.normalise_f32(c["pts"], c["bound"])
    assert np.all(diff[(raw != 0.0) & (raw != 1.0)] == 0.0)              # ... and only on the faces of the box


def test_bounds_follow_their_derivations():
    assert H.fixed_point_step(1.0) == 2.0 ** -24 and H.fixed_point_step(0.75) == 2.0 ** -25 and H.fixed_point_step(1e6) == 2.0 ** -5
    for amax in (1e-6, 0.3, 1.0, 7.5, 1e6):
        step = H.fixed_point_step(amax)
        assert amax / step < 2.0 ** 25 <= 2.0 * amax / step and step <= amax * 2.0 ** -24
    assert H.fixed_point_step(0.0) == 0.0
    count, abs_sum = np.asarray([0, 3]), np.asarray([[0.0, 0.0], [2.0, 4.0]])
    assert np.array_equal(H.scatter_float_bound(count, abs_sum, 512)[0], [0.0, 0.0])
    assert np.array_equal(H.scatter_float_bound(count, abs_sum, 512)[1], (3 + H.C_TERM + 1) * H.U * abs_sum[1])
    fixed = H.scatter_fixed_bound(count, abs_sum, 1.0, 5000)
    assert np.array_equal(fixed[1], 3 * 2.0 ** -24 + (H.C_TERM + 1 + 2) * H.U * abs_sum[1]) and np.array_equal(fixed[0], [0.0, 0.0])
    assert np.array_equal(H.forward_bound(np.asarray([2.0])), [12 * H.U * 2.0])
    assert np.array_equal(H.input_gradient_bound(np.asarray([1.0]), 16), [32 * H.U])
    assert np.array_equal(H.input_gradient_bound(np.asarray([1.0]), 16, np.asarray([3.0]), initial_adds=16), [(32 + 16 * 4) * H.U])
    assert H.worst_fraction([1.0, 5.0], [2.0, 0.0]) == 0.5
    # the speculative form's overflow records: two more roundings per record on top of the counted form's bound
    spec = H.spec_overflow_bound(count, abs_sum, 1.0, 5000)
    assert np.all(spec >= fixed) and np.array_equal(spec[0], [0.0, 0.0])
    assert np.array_equal(spec[1], fixed[1] + 2.0 * 3 * H.U * abs_sum[1])
    assert np.array_equal(H.planned_capacities([0, 7, 8, 1000]), [64, 71, 73, 1189])


@pytest.mark.parametrize("name", TABLES)
def test_bin_counts_cover_every_live_record(cases, name):
    """sum of the bins = 8 records per live (row, level); three tables: the bins of virtual level table * L + level"""
    c = cases[name]
    ref, d_feat = c["ref"], c["d_feat"]
    n_levels = ref.n_levels
    live = (d_feat.reshape(ref.n, n_levels, 2) != 0).any(axis=-1)
    assert live[::7].sum() == 0 and live.sum() == (ref.n - len(range(0, ref.n, 7))) * n_levels
    bins = H.bin_counts(ref, d_feat)
    slices = H.level_slices(c["levels"])
    assert bins.shape == (sum(slices),) and bins.dtype == np.int64
    assert int(bins.sum()) == 8 * int(live.sum())
    if name == "instant_l16_t19":
        assert sum(slices) == 1592
    # per level: exactly that level's records
    first = np.concatenate([[0], np.cumsum(slices)])
    for li in range(n_levels):
        assert int(bins[first[li]:first[li + 1]].sum()) == 8 * int(live[:, li].sum())
    # a level whose gradient columns are zero everywhere has no record
    d2 = d_feat.copy()
    d2[:, 0:2] = 0.0
    assert int(H.bin_counts(ref, d2)[:slices[0]].sum()) == 0
    # a pair with ONE non-zero component is live
    d3 = np.zeros_like(d_feat)
    d3[3, 1] = 1e-30
    assert int(H.bin_counts(ref, d3).sum()) == 8
    three = np.stack([d_feat, d2, np.zeros_like(d_feat)])
    stacked = H.bin_counts(ref, three)
    assert np.array_equal(stacked, np.concatenate([bins, H.bin_counts(ref, d2), np.zeros_like(bins)]))


def test_bin_counts_equal_a_brute_force_loop():
    n_levels, log2_t, base, pls, bound = 5, 14, 16, 1.5, 1.5         # 4920-entry dense level 0 (two slices), hashed levels of four
    levels = O.hash_grid_levels(n_levels, log2_t, base, pls)
    pts = H.random_batch(bound, 40, 3)
    rng = np.random.default_rng(4)
    d_feat = rng.standard_normal((40, 2 * n_levels))
    d_feat[::3] = 0.0
    d_feat[5, 2:4] = 0.0
    ref = H.HashReference(pts, levels, bound)
    slices = H.level_slices(levels)
    assert max(slices) > 1
    want = [np.zeros(s, dtype=np.int64) for s in slices]
    for p in range(40):
        for li in range(n_levels):
            if d_feat[p, 2 * li] == 0.0 and d_feat[p, 2 * li + 1] == 0.0:
                continue
            for k in range(8):
                want[li][(int(ref.idx[p, li, k]) - int(levels[li].offset)) // 4096] += 1
    assert np.array_equal(H.bin_counts(ref, d_feat), np.concatenate(want))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n,n_levels", [(1, 16), (33, 12), (129, 12), (200, 1), (128, 3), (300, 4)])
def test_decode_nat_round_trips_an_independent_encoder(n, n_levels, dtype):
    """the encoder here walks (row, feature) and places every word by the address arithmetic of the layout comment;
    the decoder reshapes by the tile structure -- two restatements that must agree"""
    rng = np.random.default_rng(n + n_levels)
    n_pad, n_ks = H.nat_padded_rows(n), (2 * n_levels + 15) // 16
    assert n_pad % 128 == 0 and n_pad - 128 < n <= n_pad
    feat = rng.standard_normal((n, 2 * n_levels)).astype(np.float32)
    words = H.round_to_bf16_words(feat) if dtype == "bf16" else H.round_to_f16_words(feat)
    poison = 0x7B7B
    image = np.full(n_pad * 16 * n_ks, poison, dtype=np.uint16)
    touched = np.zeros(image.shape, dtype=bool)
    for p in range(n_pad):
        src = min(p, n - 1)
        for f in range(2 * n_levels):
            tile, col, ks, half, j = p // 32, p % 32, f // 16, (f // 8) % 2, f % 8
            at = ((tile * n_ks + ks) * 64 + 2 * col + half) * 8 + j
            image[at] = words[src, f]
            touched[at] = True
    values, written = H.decode_nat(image, n, n_levels, dtype)
    assert values.shape == written.shape == (n_pad, 16 * n_ks)
    assert np.array_equal(touched, H.nat_written_words(n, n_levels))
    rows = H.nat_rows(image, n, n_levels)
    assert np.array_equal(rows[:n, :2 * n_levels], words) and np.all(rows[~written] == poison)
    assert np.all(rows[n:, :2 * n_levels] == words[n - 1])
    if dtype == "bf16":
        expect = torch.from_numpy(feat).to(torch.bfloat16).float().numpy()
    else:
        expect = torch.from_numpy(feat).to(torch.float16).float().numpy()
    assert np.array_equal(values[:n, :2 * n_levels], expect)
