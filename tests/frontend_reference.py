"""Host restatement of the ray front end, in numpy / torch / Python integers, for tests/test_gpu_frontend.py.

Nothing here calls the HIP library.  Every function states one thing the kernels promise:

* the counter-based generator ("squares", B. Widynski, "Squares: A Fast Counter-Based RNG", arXiv:2004.06278, the
  four-round 32-bit form) with the project's key derivation (splitmix64 of the seed, forced odd) and stream layout:
  word ``(counter << 40) + index``; jitter draws sit at index = global sample number, the pixel draw of global ray r at
  ``2^39 + 2 r`` and ``2^39 + 2 r + 1`` (bit 39 keeps it clear of the jitter stream, whose indices stay below 2^39 there);
* the pixel draw ``umulhi(r64, n_pixels)`` and its decomposition (image, row, column) with the column fastest;
* the ray of a pixel and the composited target, in fp32 with one rounding per operation, in the order
  project-nerf_amd/csrc/sample.hip documents (no +0.5 pixel centre, -y, -z, three products summed left to right);
* the Part 4 coordinate / time noise: four fp64 normals per sample from the four uniforms at 4 g .. 4 g + 3 of the noise
  stream (key of ``seed ^ 0x6e6f697365``), Box-Muller with u1 floored at 2^-24;
* the forward CDF of the inverse-CDF resampler in fp64, and the bound its fp32 kernel has to meet in the CDF's own units.
"""
import numpy as np
import torch

from oracle import nerf_oracle as O

MASK64 = (1 << 64) - 1
PIXEL_BIT = 1 << 39
NOISE_SEED_XOR = 0x6e6f697365
U24 = 2.0 ** -24


# --------------------------------------------------------------------------------------------------- generator
def squares_key(seed):
    """splitmix64 finaliser of ``seed + golden ratio``, forced odd (Python integers, modulo 2^64)"""
    key = (int(seed) + 0x9E3779B97F4A7C15) & MASK64
    key = ((key ^ (key >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    key = ((key ^ (key >> 27)) * 0x94D049BB133111EB) & MASK64
    return (key ^ (key >> 31)) | 1


def squares32_int(ctr, key):
    """one 32-bit draw in Python integers: four rounds of square-and-add, the halves swapped after the first three"""
    y = x = (ctr * key) & MASK64
    z = (y + key) & MASK64
    for add in (y, z, y):
        x = (x * x + add) & MASK64
        x = (x >> 32) | ((x << 32) & MASK64)
    return ((x * x + z) & MASK64) >> 32


def squares32(ctr, key):
    """the same on a uint64 array of counters (wrap-around arithmetic); returns uint64 values below 2^32"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    k = np.uint64(key)
    s32 = np.uint64(32)
    with np.errstate(over="ignore"):
        y = ctr * k
        z = y + k
        x = y.copy()
        for add in (y, z, y):
            x = x * x + add
            x = (x >> s32) | (x << s32)
        return (x * x + z) >> s32


def stream_word(counter, index):
    """uint64 generator counter of draw ``index`` (< 2^40) of step ``counter`` (< 2^24)"""
    index = np.asarray(index, dtype=np.uint64)
    return np.uint64(int(counter) << 40) + index


def squares_uniform(counter, index, key):
    """fp32 uniform in [0, 1) with 24 bits: the top 24 bits of the draw times 2^-24"""
    bits = squares32(stream_word(counter, index), key) >> np.uint64(8)
    return (bits.astype(np.float32) * np.float32(U24)).astype(np.float32)


def umulhi(a, b):
    return (int(a) * int(b)) >> 64


def pixel_draw(counter, global_ray, key, n_pixels):
    """flat pixel index in [0, n_pixels) of every global ray: the high word of r64 * n_pixels, r64 from the two draws at
    ``(counter << 40) + 2^39 + 2 ray`` (high half) and the word after it (low half); exact Python integers"""
    ray = np.asarray(global_ray, dtype=np.uint64).reshape(-1)
    c0 = stream_word(counter, np.uint64(PIXEL_BIT) + np.uint64(2) * ray)
    hi, lo = squares32(c0, key), squares32(c0 + np.uint64(1), key)
    return np.array([umulhi((int(h) << 32) | int(l), n_pixels) for h, l in zip(hi, lo)], dtype=np.int64)


def pixel_of(flat, H, W):
    """(image, row, column) of a flat index over [n, H, W]: the column runs fastest"""
    flat = np.asarray(flat, dtype=np.int64)
    return flat // (H * W), (flat // W) % H, flat % W


# --------------------------------------------------------------------------------------------------- rays, targets
def rays_of_pixels(poses, im, py, px, H, W, focal, scene_scale):
    """(origins [n,3], unit directions [n,3]) in fp32, one rounding per operation"""
    f32 = np.float32
    c2w = np.asarray(poses, dtype=f32)[np.asarray(im)]
    focal = f32(focal)
    x = (np.asarray(px).astype(f32) - f32(W * 0.5)) / focal
    y = -((np.asarray(py).astype(f32) - f32(H * 0.5)) / focal)
    z = f32(-1.0)
    d = np.stack([(c2w[:, i, 0] * x + c2w[:, i, 1] * y) + c2w[:, i, 2] * z for i in range(3)], axis=-1).astype(f32)
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)
    o = c2w[:, :3, 3]
    if float(scene_scale) != 1.0:
        o = o * f32(scene_scale)
    return o.astype(f32), (d / nrm[:, None]).astype(f32)


def composite_target(rgba, bg):
    """rgb * a + bg * (1 - a) in fp32, every product and sum rounded"""
    rgba, bg = np.asarray(rgba, dtype=np.float32), np.asarray(bg, dtype=np.float32)
    a = rgba[:, 3:4]
    rest = np.float32(1.0) - a
    return (rgba[:, :3] * a + bg[None, :] * rest).astype(np.float32)


def jitter_uniforms(counter, first_ray, n_rays, n_samples, key):
    """[n_rays, n_samples] fp32 uniforms of the depth jitter: draw index = global sample number"""
    g = np.uint64(int(first_ray) * int(n_samples)) + np.arange(int(n_rays) * int(n_samples), dtype=np.uint64)
    return squares_uniform(counter, g, key).reshape(n_rays, n_samples)


def train_batch_reference(frames, poses, focal, scene_scale, bg, seed, counter, first_ray, batch, n_samples, near, far, perturb):
    """what nerf_train_batch_shard promises for rays [first_ray, first_ray + batch) of the global batch: dict of numpy arrays
    (flat pixel, origins, directions, rgba, target) and the depths as a torch tensor"""
    n, H, W, _ = frames.shape
    key = squares_key(seed)
    flat = pixel_draw(counter, int(first_ray) + np.arange(batch, dtype=np.uint64), key, n * H * W)
    im, py, px = pixel_of(flat, H, W)
    o, d = rays_of_pixels(poses, im, py, px, H, W, focal, scene_scale)
    rgba = np.asarray(frames, dtype=np.float32)[im, py, px]
    u = torch.from_numpy(jitter_uniforms(counter, first_ray, batch, n_samples, key)) if perturb else None
    z = O.stratified_depths(near, far, n_samples, batch, bool(perturb), u=u).contiguous()
    return dict(flat=flat, o=o, d=d, rgba=rgba, target=None if bg is None else composite_target(rgba, bg), z=z)


def random_poses(n, rng):
    """[n,4,4] fp32 camera-to-world matrices: a random orthonormal frame (QR of a Gaussian matrix) and a random origin"""
    out = np.zeros((n, 4, 4), dtype=np.float32)
    for i in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        out[i, :3, :3] = q
        out[i, :3, 3] = rng.standard_normal(3) * 3.0
        out[i, 3, 3] = 1.0
    return out


# --------------------------------------------------------------------------------------------------- Part 4 noise
def noise_key(seed):
    return squares_key(int(seed) ^ NOISE_SEED_XOR)


def normal_noise(counter, global_sample, key):
    """[n,4] fp64 standard normals of the samples with the given GLOBAL indices: columns 0..2 perturb x, column 3 the time.
    Sample g owns the uniforms at 4 g .. 4 g + 3; (z0, z1) = r(u[0]) (cos, sin)(2 pi u[1]), (z2, z3) the same from u[2], u[3]"""
    g = np.asarray(global_sample, dtype=np.uint64).reshape(-1)
    u = np.stack([squares_uniform(counter, np.uint64(4) * g + np.uint64(k), key) for k in range(4)], axis=-1).astype(np.float64)
    out = np.empty((g.shape[0], 4), dtype=np.float64)
    for pair in range(2):
        r = np.sqrt(-2.0 * np.log(np.maximum(u[:, 2 * pair], U24)))
        ang = 2.0 * np.pi * u[:, 2 * pair + 1]
        out[:, 2 * pair], out[:, 2 * pair + 1] = r * np.cos(ang), r * np.sin(ang)
    return out


# --------------------------------------------------------------------------------------------------- inverse-CDF resampler
# (n_coarse, n_fine): the CDF entries per lane go 1 -> 2 at S = 66, 2 -> 3 at 130, 3 -> 4 at 194; (256, 768) sorts the largest
# array the kernel takes, (100, 156) fills its power of two exactly, (100, 157) is mostly padding
PDF_SHAPES = [(3, 1), (3, 5), (4, 7), (64, 128), (65, 64), (66, 64), (129, 64), (130, 100), (193, 64), (194, 300), (256, 768),
              (256, 1), (100, 156), (100, 157)]
PDF_RAYS = 7


def pdf_case(S, NF, R=PDF_RAYS):
    """(z [R,S] strictly increasing stratified-jittered depths, w [R,S] = rand^4 with an all-zero first ray, u [R,NF] sorted)"""
    gen = torch.Generator().manual_seed(1000 * S + NF)
    z = O.stratified_depths(2.0, 6.0, S, R, True, u=torch.rand(R, S, generator=gen)).contiguous()
    assert bool((z[:, 1:] > z[:, :-1]).all())
    w = torch.rand(R, S, generator=gen) ** 4
    w[0] = 0.0
    u = torch.sort(torch.rand(R, NF, generator=gen), dim=-1).values.contiguous()
    return z, w.contiguous(), u


def _pdf_tables(z, w):
    """fp64 (bins [R,S-1], cdf [R,S-1]) of fp32 inputs: mid-points, pdf = interior weights + fp32(1e-5), normalised"""
    z, w = np.asarray(z, dtype=np.float64), np.asarray(w, dtype=np.float64)
    bins = 0.5 * (z[:, 1:] + z[:, :-1])
    pdf = w[:, 1:-1] + np.float64(np.float32(1e-5))
    cdf = np.concatenate([np.zeros_like(pdf[:, :1]), np.cumsum(pdf, axis=-1)], axis=-1) / pdf.sum(-1, keepdims=True)
    return bins, cdf


def _bin_of(table, x):
    """index k of the last table entry <= x per row, clipped to a bin [k, k+1] of the table"""
    k = (x[:, :, None] >= table[:, None, :]).sum(-1) - 1
    return np.clip(k, 0, table.shape[1] - 2)


def pdf_forward_cdf(z, w, v):
    """F(v) [R,N] in fp64: the piecewise-linear CDF over the mid-point bins, 0 before the first and 1 after the last"""
    bins, cdf = _pdf_tables(z, w)
    v = np.asarray(v, dtype=np.float64)
    k = _bin_of(bins, v)
    take = lambda a, i: np.take_along_axis(a, i, axis=1)
    b0, b1, c0, c1 = take(bins, k), take(bins, k + 1), take(cdf, k), take(cdf, k + 1)
    return np.clip(c0 + (v - b0) / (b1 - b0) * (c1 - c0), c0, c1)


def pdf_tolerance(z, w, u):
    """(tol, mass) [R,N]: the bound on |F(v_kernel) - u| of a draw u and the mass of the bin it lands in.
    tol = (S-2) 2^-23 [fp32 prefix sum and normalisation] + slope_k * 4 * 2^-23 * |v| [four roundings of the interpolated
    depth, seen through the bin's slope mass_k / width_k] + (1e-5 if mass_k < 2e-5) [the kernel's rule denom < 1e-5 -> 1, on
    either side of its threshold]; v is the exact inverse of u"""
    bins, cdf = _pdf_tables(z, w)
    u = np.asarray(u, dtype=np.float64)
    S = bins.shape[1] + 1
    k = _bin_of(cdf, u)
    take = lambda a, i: np.take_along_axis(a, i, axis=1)
    b0, b1, c0, c1 = take(bins, k), take(bins, k + 1), take(cdf, k), take(cdf, k + 1)
    mass, width = c1 - c0, b1 - b0
    v = b0 + np.clip((u - c0) / mass, 0.0, 1.0) * width
    tol = (S - 2) * 2.0 ** -23 + mass / width * 4.0 * 2.0 ** -23 * np.abs(v) + np.where(mass < 2e-5, 1e-5, 0.0)
    return tol, mass


def fine_of_merged(out, z):
    """the values of the sorted rows ``out`` [R, S+N] left after taking every coarse depth z [R,S] (strictly increasing rows)
    out once, bit for bit: [R,N] in order, or None when a coarse depth is missing"""
    out, z = np.asarray(out), np.asarray(z)
    eq = out[:, :, None] == z[:, None, :]                       # [R, T, S]
    if not eq.any(axis=1).all():
        return None
    first = eq.argmax(axis=1)                                   # [R, S]: the first position of each coarse depth
    keep = np.ones(out.shape, dtype=bool)
    np.put_along_axis(keep, first, False, axis=1)
    if not (keep.sum(-1) == out.shape[1] - z.shape[1]).all():
        return None
    return out[keep].reshape(out.shape[0], out.shape[1] - z.shape[1])
