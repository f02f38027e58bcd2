"""tests/frontend_reference.py against facts that do not come from it: integer identities of the generator and of the pixel
draw, the layout of the draw streams, the oracle's stratified depths and inverse CDF, and an fp32 numpy emulation of the
resampling kernel (lane-blocked prefix sum in rows of 16, binary search, interpolation) on which the bound of
``pdf_tolerance`` has to hold with room, at the shapes the GPU test runs."""
import numpy as np
import pytest
import torch

import frontend_reference as F
from oracle import nerf_oracle as O


# --------------------------------------------------------------------------------------------------- generator
def test_squares_key_is_odd_and_spreads_the_seed():
    keys = [F.squares_key(s) for s in list(range(64)) + [2 ** 32, 2 ** 63, 2 ** 64 - 1, F.NOISE_SEED_XOR]]
    assert all(k & 1 and 0 < k < 2 ** 64 for k in keys)
    assert len(set(keys)) == len(keys)
    assert F.noise_key(7) == F.squares_key(7 ^ 0x6e6f697365) != F.squares_key(7)


def test_vector_generator_equals_python_integers():
    rng = np.random.default_rng(0)
    key = F.squares_key(12345)
    ctr = np.concatenate([rng.integers(0, 2 ** 63, size=200, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                          np.array([0, 1, 2 ** 39, 2 ** 40 - 1, 2 ** 64 - 1, (2 ** 24 - 1) << 40], dtype=np.uint64)])
    got = F.squares32(ctr, key)
    assert got.dtype == np.uint64 and int(got.max()) < 2 ** 32
    assert [int(g) for g in got] == [F.squares32_int(int(c), key) for c in ctr]
    # uniforms: multiples of 2^-24 in [0, 1), from the top 24 bits
    u = F.squares_uniform(5, np.arange(4096), key)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert np.array_equal(u.astype(np.float64) * 2 ** 24, (F.squares32(F.stream_word(5, np.arange(4096)), key) >> np.uint64(8)).astype(np.float64))
    assert abs(float(u.mean()) - 0.5) < 0.02                       # 4096 draws: sigma of the mean 0.0045


def test_umulhi_equals_the_split_product():
    rng = np.random.default_rng(1)
    m32 = (1 << 32) - 1
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 2 ** 63, size=(300, 2), dtype=np.uint64) * np.uint64(2) + np.uint64(1)]
    pairs += [(2 ** 64 - 1, 2 ** 64 - 1), (2 ** 64 - 1, 1), (0, 5), (2 ** 32, 2 ** 32), (2 ** 64 - 1, 105)]
    for a, b in pairs:
        a1, a0, b1, b0 = a >> 32, a & m32, b >> 32, b & m32
        mid = a1 * b0 + ((a0 * b0) >> 32)
        mid2 = a0 * b1 + (mid & m32)
        assert F.umulhi(a, b) == a1 * b1 + (mid >> 32) + (mid2 >> 32)


@pytest.mark.parametrize("n_pixels", [1, 2, 3, 105, 72])
def test_pixel_draw_range_and_decomposition(n_pixels):
    key = F.squares_key(3)
    flat = F.pixel_draw(9, np.arange(2000), key, n_pixels)
    assert flat.min() == 0 and flat.max() == n_pixels - 1          # both ends (2000 draws over at most 105 values)
    # the first ray by hand
    c0 = (9 << 40) + (1 << 39)
    r64 = (F.squares32_int(c0, key) << 32) | F.squares32_int(c0 + 1, key)
    assert int(flat[0]) == (r64 * n_pixels) >> 64
    # a global ray number is all that matters, wherever the call starts
    assert np.array_equal(F.pixel_draw(9, 1500 + np.arange(500), key, n_pixels), flat[1500:])
    if n_pixels == 105:
        im, py, px = F.pixel_of(flat, 5, 7)
        assert np.array_equal((im * 5 + py) * 7 + px, flat) and im.max() == 2 and py.max() == 4 and px.max() == 6
        im2, py2, px2 = F.pixel_of(flat, 7, 5)                     # rows and columns are not interchangeable
        assert not np.array_equal(py, py2)


def test_streams_do_not_meet():
    """words of the generator: jitter draws of train_batch take [c << 40, (c << 40) + 2^39), its pixel draws the upper
    half of the same 2^40 block; the noise of a sample ends below 2^40 when samples stay below 2^38"""
    def block(c, lo, hi):
        return int(F.stream_word(c, lo)), int(F.stream_word(c, hi))
    last = None
    for c in (0, 1, 2, 2 ** 24 - 2, 2 ** 24 - 1):
        j_lo, j_hi = block(c, 0, 2 ** 39 - 1)
        p_lo, p_hi = block(c, F.PIXEL_BIT + 2 * 0, F.PIXEL_BIT + 2 * (2 ** 38 - 1) + 1)
        assert j_lo == c << 40 and j_lo <= j_hi < p_lo <= p_hi == ((c + 1) << 40) - 1 < 2 ** 64
        assert last is None or last < j_lo
        last = p_hi
        n_hi = int(F.stream_word(c, 4 * (2 ** 38 - 1) + 3))
        assert n_hi == p_hi                                        # the last noise draw of the last admissible sample
    # the words are 64-bit: nothing is lost above bit 31 of the index
    key = F.squares_key(1)
    a, b = F.squares_uniform(0, np.array([5, 5 + 2 ** 32, 5 + 2 ** 39]), key), F.squares_uniform(1, np.array([5]), key)
    assert len({float(x) for x in a} | {float(b[0])}) == 4


def test_generated_jitter_stays_inside_the_strata():
    key = F.squares_key(11)
    for R, S, first in ((5, 2, 0), (7, 5, 3), (3, 64, 100)):
        u = F.jitter_uniforms(2 ** 24 - 1, first, R, S, key)
        assert np.array_equal(u, F.jitter_uniforms(2 ** 24 - 1, 0, first + R, S, key)[first:])     # global numbering
        z = O.stratified_depths(2.0, 6.0, S, R, True, u=torch.from_numpy(u))
        plain = O.stratified_depths(2.0, 6.0, S, R, False)
        mids = 0.5 * (plain[:, 1:] + plain[:, :-1])
        lo, hi = torch.cat([plain[:, :1], mids], -1), torch.cat([mids, plain[:, -1:]], -1)
        assert bool((z >= lo).all()) and bool((z <= hi).all())


def test_normal_noise_uses_four_uniforms_per_sample():
    key = F.noise_key(5)
    g = np.array([0, 1, 41 * 17, 2 ** 38 - 1], dtype=np.uint64)
    n = F.normal_noise(3, g, key)
    u = np.stack([F.squares_uniform(3, np.uint64(4) * g + np.uint64(k), key) for k in range(4)], -1).astype(np.float64)
    # (z0, z1) and (z2, z3) are points of radius sqrt(-2 ln u) at angle 2 pi u'
    for p in range(2):
        r2 = n[:, 2 * p] ** 2 + n[:, 2 * p + 1] ** 2
        np.testing.assert_allclose(r2, -2.0 * np.log(np.maximum(u[:, 2 * p], 2.0 ** -24)), rtol=1e-12)
        ang = np.arctan2(n[:, 2 * p + 1], n[:, 2 * p]) / (2 * np.pi) % 1.0
        np.testing.assert_allclose(ang, u[:, 2 * p + 1], atol=1e-12)
    big = F.normal_noise(0, np.arange(50000), key)
    assert abs(float(big.mean())) < 0.02 and abs(float(big.var()) - 1.0) < 0.02


def test_rays_of_pixels_against_a_float64_evaluation():
    rng = np.random.default_rng(2)
    H, W, focal = 5, 7, 6.25
    poses = F.random_poses(3, rng)
    im, py, px = rng.integers(0, 3, 200), rng.integers(0, H, 200), rng.integers(0, W, 200)
    o, d = F.rays_of_pixels(poses, im, py, px, H, W, focal, 0.5)
    cam = np.stack([(px - W * 0.5) / focal, -(py - H * 0.5) / focal, -np.ones(200)], -1)
    d64 = np.einsum("nij,nj->ni", poses[im, :3, :3].astype(np.float64), cam)
    d64 /= np.linalg.norm(d64, axis=-1, keepdims=True)
    assert o.dtype == d.dtype == np.float32
    assert np.abs(d - d64).max() < 3e-7
    assert np.array_equal(o, poses[im, :3, 3] * np.float32(0.5))
    assert np.array_equal(F.rays_of_pixels(poses, im, py, px, H, W, focal, 1.0)[0], poses[im, :3, 3])


# --------------------------------------------------------------------------------------------------- inverse CDF
def test_forward_cdf_inverts_the_oracle_in_float64():
    for S, NF in ((3, 5), (64, 128), (130, 100)):
        z, w, u = F.pdf_case(S, NF)
        out = O.sample_pdf(z.double(), w.double(), NF, u.double()).numpy()
        fine = F.fine_of_merged(out, z.double().numpy())
        assert fine is not None and fine.shape == (F.PDF_RAYS, NF)
        err = np.abs(F.pdf_forward_cdf(z.numpy(), w.numpy(), fine) - u.double().numpy())
        _, mass = F.pdf_tolerance(z.numpy(), w.numpy(), u.numpy())
        # the oracle adds the double 1e-5 where the kernel (and the forward CDF) add fp32(1e-5): 2.5e-8 of the floor; bins
        # lighter than its threshold 1e-5 are not inverted at all (denominator 1)
        assert float(err[mass >= 1.1e-5].max()) < 1e-9
        assert float(err.max()) < 1.1e-5


def emulate_sample_pdf(z, w, u, fma):
    """nerf_sample_pdf in fp32 numpy, row-vectorised: lane l of 64 owns the K consecutive pdf entries l K .. l K + K - 1,
    sums them in order, the 64 sums are scanned in rows of 16 (shifts 1, 2, 4, 8) with the row carries r0, r0 + r1,
    r0 + r1 + r2; cdf = exclusive prefix / total; binary search for the first entry > u; linear interpolation between the
    two mid-points (``fma``: product and sum rounded once)."""
    f32 = np.float32
    z, w, u = z.astype(f32), w.astype(f32), u.astype(f32)
    R, S = z.shape
    nb = S - 1
    K = (nb + 63) // 64
    local = np.zeros((R, 64 * K), dtype=f32)
    local[:, :S - 2] = w[:, 1:-1] + f32(1e-5)
    local = local.reshape(R, 64, K)
    lane_sum = np.zeros((R, 64), dtype=f32)
    for k in range(K):
        lane_sum = lane_sum + local[:, :, k]
    v = lane_sum.reshape(R, 4, 16).copy()
    for sh in (1, 2, 4, 8):
        shifted = np.zeros_like(v)
        shifted[:, :, sh:] = v[:, :, :-sh]
        v = v + shifted
    r0, r1, r2 = v[:, 0, 15], v[:, 1, 15], v[:, 2, 15]
    carry = np.stack([np.zeros_like(r0), r0, r0 + r1, (r0 + r1) + r2], axis=1)
    incl = (v + carry[:, :, None]).reshape(R, 64)
    total = incl[:, 63:64]
    run = incl - lane_sum
    cdf = np.zeros((R, 64, K), dtype=f32)
    for k in range(K):
        cdf[:, :, k] = run / total
        run = run + local[:, :, k]
    cdf = cdf.reshape(R, 64 * K)[:, :nb]
    bins = f32(0.5) * (z[:, 1:] + z[:, :-1])
    take = lambda a, i: np.take_along_axis(a, i, axis=1)
    lo, hi = np.zeros(u.shape, dtype=np.int64), np.full(u.shape, nb, dtype=np.int64)
    while bool((lo < hi).any()):
        live = lo < hi
        mid = (lo + hi) >> 1
        right = take(cdf, np.minimum(mid, nb - 1)) <= u
        lo, hi = np.where(live & right, mid + 1, lo), np.where(live & ~right, mid, hi)
    below, above = np.maximum(lo - 1, 0), np.minimum(lo, nb - 1)
    denom = take(cdf, above) - take(cdf, below)
    denom = np.where(denom < f32(1e-5), f32(1.0), denom)
    t = (u - take(cdf, below)) / denom
    b0, span = take(bins, below), take(bins, above) - take(bins, below)
    fine = (b0.astype(np.float64) + t.astype(np.float64) * span.astype(np.float64)).astype(f32) if fma else b0 + t * span
    return np.sort(np.concatenate([z, fine.astype(f32)], axis=-1), axis=-1)


@pytest.mark.parametrize("S,NF", F.PDF_SHAPES)
def test_pdf_tolerance_holds_on_the_fp32_emulation(S, NF):
    z, w, u = (t.numpy() for t in F.pdf_case(S, NF))
    tol, mass = F.pdf_tolerance(z, w, u)
    heavy = float((mass > 100.0 * tol).mean())
    worst = 0.0
    for fma in (False, True):
        out = emulate_sample_pdf(z, w, u, fma)
        fine = F.fine_of_merged(out, z)
        assert fine is not None
        worst = max(worst, float((np.abs(F.pdf_forward_cdf(z, w, fine) - u) / tol).max()))
    print(f"[pdf {S}x{NF}] error / tolerance {worst:.3f}, draws in bins heavier than 100 tol: {heavy:.3f}")
    assert worst < 1.0
    assert heavy >= 0.85


def test_a_slip_of_one_bin_breaks_the_tolerance():
    """the reason for the condition on heavy bins: moving every fine depth to the same place of the next bin is caught"""
    S, NF = 64, 128
    z, w, u = (t.numpy() for t in F.pdf_case(S, NF))
    tol, mass = F.pdf_tolerance(z, w, u)
    fine = F.fine_of_merged(emulate_sample_pdf(z, w, u, False), z)
    width = (z[:, -1:] - z[:, :1]).astype(np.float64) / (S - 1)
    bad = np.abs(F.pdf_forward_cdf(z, w, fine + width) - u) > tol
    assert float(bad.mean()) > 0.8
