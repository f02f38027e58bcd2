"""Exact corner-list reference of the multiresolution hash grid (csrc/hashgrid.hip), for the tests.

A helper module, not a test.  Plain numpy: the cell of a point is this build's fp32 definition (so the
indices are exact), everything after it is int64 / float64.  ``frac = pos - floor(pos)`` is exact in fp32
(Sterbenz), so promoting it loses nothing; weights, features and gradients are float64 products and sums.

The error bounds at the end are functions of reference-side quantities only (sums of absolute terms,
contribution counts, the launch's largest |d_feat|, the batch size).  Each docstring counts the fp32
roundings -- or restates the fixed-point record format -- the bound rests on.  ``U`` is the unit roundoff
of fp32, 2^-24: one round-to-nearest operation errs by at most ``U`` relative to its result.
"""
import math

import numpy as np

U = 2.0 ** -24

# (n_levels, log2_hashmap_size, base_resolution, per_level_scale, bound)
LEVEL_TABLES = {
    "instant_l16_t19": (16, 19, 16, 1.5, 1.5),      # the Instant-NGP default
    "deform_l12_t10": (12, 10, 16, 1.5, 1.5),       # Part 4 deformation: all levels hashed, 24 of 32 image columns written
    "single_level": (1, 19, 16, 1.5, 1.5),
    "dense_small_res": (3, 15, 4, 1.5, 1.5),        # res 4, 6, 9: all dense, 729 padded to 736, wrap at the upper faces
    "nodes_l4_t14": (4, 14, 17, 2.0, 1.0),          # level 0: scale 16 (exact nodes), 17^3 = 4913 padded to 4920 (LDS pass); level 1 hashed
}
ROW_COUNTS = (1, 31, 32, 33, 127, 128, 129)         # and the whole probe set
ONE_CELL_POINTS = 5000                              # the largest batch of the suite

HASH_PRIMES = (1, 2654435761, 805459861)
MUTATIONS = (None, "swap_axis_weights", "flip_corner_sign", "open_clamp")


def level_arrays(levels):
    """(scale fp32, res, size, offset, dense) of a level list from oracle.hash_grid_levels"""
    return (np.asarray([lv.scale for lv in levels], dtype=np.float32), [int(lv.res) for lv in levels],
            [int(lv.size) for lv in levels], [int(lv.offset) for lv in levels], [bool(lv.dense) for lv in levels])


def normalise_f32(pts, bound):
    """x01 BEFORE the clamp, in fp32 like the kernel and the module it replaces: (x + bound) / (2 bound)"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    b = np.float32(bound)
    return (pts + b) / (np.float32(2.0) * b)


def corner_lists(pts, levels, bound, mutate=None):
    """idx [n,L,8] int64 (absolute table entry), w [n,L,8] float64, frac [n,L,3] float64.
    Corner c: bit 0 -> x, bit 1 -> y, bit 2 -> z.  ``mutate`` ("swap_axis_weights"): the y and z weights
    exchanged -- a deliberately wrong reference for the sensitivity checks."""
    assert mutate in MUTATIONS
    raw = normalise_f32(pts, bound)
    x01 = np.minimum(np.maximum(raw, np.float32(0.0)), np.float32(1.0))
    scale, res, size, offset, dense = level_arrays(levels)
    n, n_levels = raw.shape[0], len(levels)
    idx = np.empty((n, n_levels, 8), dtype=np.int64)
    frac = np.empty((n, n_levels, 3), dtype=np.float64)
    for li in range(n_levels):
        pos = x01 * scale[li]                        # fp32 product, rounded ...
        pos = pos + np.float32(0.5)                  # ... then the fp32 sum, rounded (numpy never contracts the two)
        assert pos.dtype == np.float32
        cell = np.floor(pos)
        frac[:, li] = (pos - cell).astype(np.float64)             # exact
        cell = cell.astype(np.int64)
        for c in range(8):
            gx, gy, gz = cell[:, 0] + (c & 1), cell[:, 1] + ((c >> 1) & 1), cell[:, 2] + ((c >> 2) & 1)
            if dense[li]:
                e = (gx + gy * res[li] + gz * res[li] * res[li]) % size[li]
            else:
                h = ((gx * HASH_PRIMES[0]) & 0xFFFFFFFF) ^ ((gy * HASH_PRIMES[1]) & 0xFFFFFFFF) ^ ((gz * HASH_PRIMES[2]) & 0xFFFFFFFF)
                e = h % size[li]
            idx[:, li, c] = e + offset[li]
    w = axis_weights(frac, mutate).prod(axis=-1)
    return idx, w, frac


def axis_weights(frac, mutate=None):
    """[n,L,8,3] float64: the weight of corner c along each axis, frac or 1 - frac"""
    bits = np.asarray([[(c >> a) & 1 for a in range(3)] for c in range(8)], dtype=bool)       # [8,3]
    if mutate == "swap_axis_weights":                # the y bit of a corner picks its weight from the z frac and the other way round
        frac = frac[..., [0, 2, 1]]
    f = frac[:, :, None, :]
    return np.where(bits[None, None], f, 1.0 - f)


class HashReference:
    """The grid at ``pts`` [n,3] fp32 for a level list of oracle.hash_grid_levels: features, table gradient and
    input gradient in float64 from one exact corner list."""

    def __init__(self, pts, levels, bound, mutate=None):
        self.pts = np.ascontiguousarray(pts, dtype=np.float32)
        self.levels, self.bound, self.mutate = levels, float(bound), mutate
        self.n, self.n_levels = self.pts.shape[0], len(levels)
        self.entries = int(levels[-1].offset + levels[-1].size)
        self.idx, self.w, self.frac = corner_lists(self.pts, levels, bound, mutate)
        raw = normalise_f32(self.pts, bound)
        # torch.clamp passes the gradient on its CLOSED interval: zero only where x01 lies strictly outside [0, 1]
        if mutate == "open_clamp":
            self.inside = (raw > 0.0) & (raw < 1.0)
        else:
            self.inside = (raw >= 0.0) & (raw <= 1.0)
        self.scale64 = np.asarray([lv.scale for lv in levels], dtype=np.float32).astype(np.float64)
        self.two_b64 = float(np.float32(2.0) * np.float32(bound))

    def features(self, table64):
        """[n, 2L] float64; leaves ``abs_terms`` = sum over the corners of |w v| per output"""
        table64 = np.asarray(table64, dtype=np.float64)
        terms = self.w[..., None] * table64[self.idx]                # [n,L,8,2]
        self.abs_terms = np.abs(terms).sum(axis=2).reshape(self.n, -1)
        return terms.sum(axis=2).reshape(self.n, -1)

    def table_gradient(self, d_feat64):
        """(grad [E,2] float64, count [E] contributions per entry from rows with a non-zero gradient,
        abs_sum [E,2] = sum |w g| per entry)"""
        g = np.asarray(d_feat64, dtype=np.float64).reshape(self.n, self.n_levels, 1, 2)
        contrib = (self.w[..., None] * g).reshape(-1, 2)
        flat = self.idx.reshape(-1)
        grad = np.zeros((self.entries, 2), dtype=np.float64)
        abs_sum = np.zeros((self.entries, 2), dtype=np.float64)
        np.add.at(grad, flat, contrib)
        np.add.at(abs_sum, flat, np.abs(contrib))
        live = np.broadcast_to((g != 0.0).any(axis=-1), self.idx.shape).reshape(-1)
        count = np.bincount(flat[live], minlength=self.entries).astype(np.int64)
        return grad, count, abs_sum

    def input_gradient(self, table64, d_feat64):
        """[n,3] float64: scale_l / (2 bound) * sum_corners (g . v) (+-1 along a) prod_{b != a} w_b, summed over the
        levels; zero on an axis whose x01 is strictly outside [0, 1].  Leaves ``abs_input_terms`` [n,3], the same
        sum with |g0 v0| + |g1 v1| and without the signs."""
        table64 = np.asarray(table64, dtype=np.float64)
        g = np.asarray(d_feat64, dtype=np.float64).reshape(self.n, self.n_levels, 1, 2)
        v = table64[self.idx]                                        # [n,L,8,2]
        gv = (g * v).sum(axis=-1)                                    # [n,L,8]
        gv_abs = np.abs(g * v).sum(axis=-1)
        wa = axis_weights(self.frac, self.mutate)                    # [n,L,8,3]
        sign = np.asarray([[1.0 if (c >> a) & 1 else -1.0 for a in range(3)] for c in range(8)])
        if self.mutate == "flip_corner_sign":
            sign[3, 0] = -sign[3, 0]
        out = np.zeros((self.n, 3))
        out_abs = np.zeros((self.n, 3))
        s = (self.scale64 / self.two_b64)[None, :]
        for a in range(3):
            others = [b for b in range(3) if b != a]
            other = wa[..., others[0]] * wa[..., others[1]]
            out[:, a] = ((gv * sign[None, None, :, a] * other).sum(axis=2) * s).sum(axis=1)
            out_abs[:, a] = ((gv_abs * other).sum(axis=2) * s).sum(axis=1)
        out = np.where(self.inside, out, 0.0)
        self.abs_input_terms = np.where(self.inside, out_abs, 0.0)
        return out


# --------------------------------------------------------------------------------------------- operand images
def _nat_ksteps(n_levels):
    return (2 * n_levels + 15) // 16


def nat_padded_rows(n):
    return (n + 127) // 128 * 128


def nat_rows(words, n, n_levels):
    """The 16-bit words of an operand image as rows [n_pad, 16 n_ks] (column = feature), from the documented tile
    structure [32-point tile][k-step][lane = (column of the tile, half)][8]: a lane holds eight consecutive
    features, the two halves of a k-step hold features 0..7 and 8..15 of its sixteen."""
    n_pad, n_ks = nat_padded_rows(n), _nat_ksteps(n_levels)
    words = np.asarray(words).reshape(-1)[: n_pad * 16 * n_ks]
    tiles = words.reshape(n_pad // 32, n_ks, 32, 2, 8)              # [tile][k-step][col][half][8]
    return tiles.transpose(0, 2, 1, 3, 4).reshape(n_pad, 16 * n_ks)


def nat_written_words(n, n_levels):
    """boolean map over the image's WORDS (image order) of what the forward writes: features below 2 L of every
    row of the padded image"""
    n_pad, n_ks = nat_padded_rows(n), _nat_ksteps(n_levels)
    feature = (16 * np.arange(n_ks)[:, None, None, None] + 8 * np.arange(2)[None, None, :, None] + np.arange(8)[None, None, None, :])
    m = np.broadcast_to(feature < 2 * n_levels, (n_pad // 32, n_ks, 32, 2, 8))
    return np.ascontiguousarray(m).reshape(-1)


def decode_nat(image, n, n_levels, dtype):
    """(values [n_pad, 16 n_ks] float32, written [n_pad, 16 n_ks] bool) of an operand image given as 16-bit words;
    ``dtype`` "bf16" or "fp16".  Unwritten columns decode to whatever the buffer held."""
    rows = nat_rows(np.asarray(image).view(np.uint16), n, n_levels)
    if dtype == "bf16":
        values = (rows.astype(np.uint32) << 16).view(np.float32)
    else:
        assert dtype == "fp16"
        values = np.ascontiguousarray(rows).view(np.float16).astype(np.float32)
    written = np.broadcast_to(np.arange(rows.shape[1])[None, :] < 2 * n_levels, rows.shape)
    return values, written


def round_to_bf16_words(x):
    """round-to-nearest-even bf16 bit patterns of finite fp32 values"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def round_to_f16_words(x):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


# --------------------------------------------------------------------------------------------- probes
def probe_points(levels, bound, seed=0):
    """[P,3] fp32: the places where the clamp's closed interval, the dense-level wrap and the weight products can go
    wrong, then random points.  Per axis: exactly +-bound, one ulp inside and outside, TWO ulps outside (see
    below), +-10 bound; -0.0; nodes (frac == 0) and cell centres of a scale-16 level; 200 points inside and 50
    outside the box.

    One ulp outside +bound is NOT outside in this build's fp32 definition: x + bound falls half-way between
    2 bound and the next float and rounds to even, to 2 bound, so x01 == 1 exactly and the gradient passes.
    The first point strictly outside on that side is two ulps away, hence the extra probe."""
    rng = np.random.default_rng(seed)
    b = np.float32(bound)
    base = np.asarray([0.31, -0.17, 0.077], dtype=np.float32) * b
    rows = []

    def per_axis(values):
        for a in range(3):
            for v in values:
                p = base.copy()
                p[a] = v
                rows.append(p)
    inf = np.float32(np.inf)
    per_axis([b, -b])
    per_axis([np.nextafter(b, -inf), np.nextafter(-b, inf)])                        # one ulp inside
    per_axis([np.nextafter(b, inf), np.nextafter(-b, -inf)])                        # one ulp outside
    per_axis([np.nextafter(np.nextafter(b, inf), inf), np.nextafter(np.nextafter(-b, -inf), -inf)])
    per_axis([np.float32(10.0) * b, np.float32(-10.0) * b])
    per_axis([np.float32(-0.0)])
    rows.append(np.asarray([-0.0, -0.0, -0.0], dtype=np.float32))
    rows.append(np.asarray([b, b, b], dtype=np.float32))
    rows.append(np.asarray([-b, -b, -b], dtype=np.float32))
    # a level of scale 16 on a box of half-width 1: x = 2 (k - 0.5) / 16 - 1 gives pos = k exactly (a node), x = 2 k / 16 - 1
    # the centre of cell k; exact in fp32 for bound 1, scaled (and merely near the nodes) for the other tables
    node = lambda k: np.float32(2.0 * (k - 0.5) / 16.0 - 1.0) * b
    centre = lambda k: np.float32(2.0 * k / 16.0 - 1.0) * b
    for k in range(1, 17):
        rows.append(np.asarray([node(k), node(17 - k), node((3 * k) % 16 + 1)], dtype=np.float32))
        rows.append(np.asarray([centre(k), centre(16 - k), centre((5 * k) % 17)], dtype=np.float32))
        rows.append(np.asarray([node(k), centre(k), base[2]], dtype=np.float32))
    inside = ((rng.random((200, 3)) * 2.0 - 1.0) * bound).astype(np.float32)
    outside = ((rng.random((50, 3)) * 2.0 - 1.0) * bound).astype(np.float32)
    which = rng.integers(1, 8, size=50)                                             # at least one axis pushed out
    push = (1.0 + rng.random((50, 3))) * bound * np.where(rng.random((50, 3)) < 0.5, -1.0, 1.0)
    for a in range(3):
        outside[:, a] = np.where((which >> a) & 1, push[:, a].astype(np.float32), outside[:, a])
    return np.ascontiguousarray(np.concatenate([np.stack(rows), inside, outside]).astype(np.float32))


def one_cell_batch(bound, n=ONE_CELL_POINTS):
    """n / 2 copies of one interior point and n / 2 copies of the corner (+b, +b, +b): two cells hold the batch"""
    b = np.float32(bound)
    interior = np.asarray([0.31, -0.17, 0.077], dtype=np.float32) * b
    half = n // 2
    return np.ascontiguousarray(np.concatenate([np.tile(interior, (half, 1)), np.tile(np.asarray([b, b, b], dtype=np.float32), (n - half, 1))]))


def random_batch(bound, n, seed):
    """seeded points, about 5 % of them outside the box on some axis"""
    rng = np.random.default_rng(seed)
    return ((rng.random((n, 3)) - 0.5) * 2.0 * bound * 1.05).astype(np.float32)


# --------------------------------------------------------------------------------------------- error bounds
C_FWD = 12


def forward_bound(abs_terms):
    """|kernel fp32 feature - reference| <= C_FWD * U * sum |w v|.

    Roundings on the path of one term: three for the weight w = (wx wy) wz (the two products, and one for its
    1 - frac factors: that subtraction is exact for frac >= 1/2 and errs by at most 2^-25 absolute below it), one for
    the product w v, seven for the adds of eight terms (the first add, to 0, is exact), one more for a compiler that
    contracts product and add into an fma whose first use rounds where the plain product did.  3 + 1 + 7 + 1 = 12
    roundings, each at most U relative to a partial result; every add is charged against the whole sum |w v|
    although it acts on a partial sum, which leaves room for the second and third 1 - frac of corner 0 (first
    order in U throughout).  The fp16 table converts to fp32 exactly, so the same bound holds against
    features(table.half())."""
    return C_FWD * U * np.asarray(abs_terms, dtype=np.float64)


C_TERM = 4          # one scatter term w g: three roundings for the weight (as in forward_bound) and one for the product


def scatter_partials(n_points):
    """partial sums one entry can meet in the float-atomic forms: the small dense levels are summed per workgroup
    of 512 points in LDS (at most 128 workgroups) and flushed with one global atomic each"""
    return min(128, (int(n_points) + 511) // 512)


def scatter_float_bound(count, abs_sum, n_points, initial=None):
    """Float-atomic and LDS scatter: |kernel - reference| <= (count + C_TERM + partials) * U * abs_sum.

    Every term carries C_TERM roundings; the ``count`` terms of an entry meet in at most count - 1 float adds
    inside a workgroup's LDS table or directly in memory, plus one add per workgroup partial; any order of those
    adds errs by at most (number of adds a term passes through) * U * abs_sum.  ``initial`` (accumulate on top of a
    non-zero d_table): one more add whose result is at most |initial| + abs_sum."""
    count = np.asarray(count, dtype=np.float64)[:, None]
    abs_sum = np.asarray(abs_sum, dtype=np.float64)
    bound = (count + C_TERM + scatter_partials(n_points)) * U * abs_sum
    if initial is not None:
        bound = bound + U * (np.abs(np.asarray(initial, dtype=np.float64)) + abs_sum)
    return bound


FIXED_BITS = 25         # magnitude bits of a record's term (26-bit signed field)
CHUNK_RECORDS = 32768   # records per work item: a bin with more is cut and its items meet through float adds


def fixed_point_step(amax):
    """Quantisation step of the binned scatter's records for a launch whose largest |d_feat| is ``amax``.

    The record packs each term w g as a 26-bit signed integer round(w g * 2^s); the shift s is chosen from the
    exponent e of amax (amax < 2^e, i.e. amax = m 2^e with 1/2 <= m < 1) as s = 25 - e, so that |w g| 2^s < 2^25,
    and clamped to [-80, 100].  One unit of the integer is 2^-s = 2^(e - 25) <= amax * 2^-24."""
    amax = float(amax)
    if not amax > 0.0:
        return 0.0
    _, e = math.frexp(float(np.float32(amax)))
    s = min(100, max(-80, FIXED_BITS - e))
    return 2.0 ** -s


def scatter_fixed_bound(count, abs_sum, amax, n_points, initial=None):
    """Binned (fixed-point) scatter: |kernel - reference| <= count * step + (C_TERM + 1 + cuts) * U * abs_sum.

    Per record: the fp32 term w g (C_TERM roundings), scaled by a power of two (exact), rounded to the nearest
    integer (half a step) and clamped to +-(2^25 - 1) (which can move a term that rounds up to 2^25 by one step):
    at most one step per record, ``count`` records per entry.  The integer sums are exact.  One rounding converts
    an item's sum to fp32 (the rescale by 2^-s is exact); a bin of more than CHUNK_RECORDS records is cut into
    ceil(8 n / CHUNK_RECORDS) items at most, which meet through one float add each.  ``initial`` (the accumulate form):
    one more add whose result is at most |initial| + abs_sum.  Terms far below the step vanish: the bound is in
    terms of the launch's amax, not of the entry's own gradients."""
    count = np.asarray(count, dtype=np.float64)[:, None]
    abs_sum = np.asarray(abs_sum, dtype=np.float64)
    cuts = (8 * int(n_points) + CHUNK_RECORDS - 1) // CHUNK_RECORDS
    bound = count * fixed_point_step(amax) + (C_TERM + 1 + cuts) * U * abs_sum
    if initial is not None:
        bound = bound + U * (np.abs(np.asarray(initial, dtype=np.float64)) + abs_sum)
    return bound


SLICE_LOG2 = 12        # a bin of the binned scatter: 4096 consecutive entries of one level (kSlice)


def level_slices(levels):
    """bins per level: ceil(size / 4096)"""
    return [(int(lv.size) + (1 << SLICE_LOG2) - 1) >> SLICE_LOG2 for lv in levels]


def bin_counts(ref, d_feat):
    """int64 [bins]: records per bin of the binned scatter for the batch of ``ref`` (a HashReference).

    A record is one corner of one (point, level) whose gradient pair is not (0, 0); its bin within the level is
    (entry - offset) >> 12.  ``d_feat`` [n, 2L]: one table, the levels' bins one after the other.  ``d_feat`` [k, n, 2L]:
    k tables of the same level structure scattered to from the same points -- the bins of virtual level table * L + level,
    in that order (plan_bins of csrc/hashgrid.hip)."""
    d = np.asarray(d_feat)
    d = d[None] if d.ndim == 2 else d
    slices = level_slices(ref.levels)
    out = []
    for k in range(d.shape[0]):
        live = (d[k].reshape(ref.n, ref.n_levels, 2) != 0).any(axis=-1)          # [n, L]
        for li, lv in enumerate(ref.levels):
            local = (ref.idx[live[:, li], li, :] - int(lv.offset)) >> SLICE_LOG2
            out.append(np.bincount(local.reshape(-1), minlength=slices[li]).astype(np.int64))
    return np.concatenate(out)


def planned_capacities(est):
    """records the speculative form plans per bin from the counts ``est`` the previous call left: est + est / 8 + 64
    (integer arithmetic, as the plan pass)"""
    est = np.asarray(est, dtype=np.int64)
    return est + (est >> 3) + 64


def spec_overflow_bound(count, abs_sum, amax, n_points):
    """Speculative binned scatter whose call was complete (status word [4] == 0):
    |kernel - reference| <= scatter_fixed_bound + 2 * count * U * abs_sum.

    A record that fits its bin is summed as in the counted form (scatter_fixed_bound, quantisation included).  A record
    that does not fit keeps its 26-bit fixed-point term (the same quantisation, already charged per record) and reaches
    d_table on its own: the integer, up to 25 magnitude bits, is converted to fp32 (one rounding, at most U times the
    term, and the terms of an entry sum to at most abs_sum), then added with one float atomic onto a partial sum of the
    entry's own terms (one rounding, at most U * abs_sum to first order).  At most ``count`` records of an entry
    overflow: 2 * count * U * abs_sum on top of the counted form's bound, whatever the order of the atomics."""
    count_col = np.asarray(count, dtype=np.float64)[:, None]
    abs_sum = np.asarray(abs_sum, dtype=np.float64)
    return scatter_fixed_bound(count, abs_sum, amax, n_points) + 2.0 * count_col * U * abs_sum


C_INPUT_TERM = 16


def input_gradient_bound(abs_input_terms, n_levels, initial=None, initial_adds=1):
    """|kernel d_pts - reference| <= (C_INPUT_TERM + n_levels) * U * abs_input_terms.

    Roundings on the path of one corner term of one level: g . v = g0 v0 + g1 v1 (two products, one add: 3, measured
    against |g0 v0| + |g1 v1|), the two 1 - frac factors (2), the products with them (2), the add into the corner
    sum (7 adds for 8 corners), the factor scale / (2 bound) (1) and the product with it (1): 16.  The levels of a
    point then meet in d_pts through at most n_levels float adds (atomics, or the ordered form's register sum).
    ``initial`` (accumulate forms, checked as result - initial): every add that lands on the memory holding the
    initial value rounds a result of at most |initial| + abs_input_terms.  The ordered form sums the levels in
    registers and adds once (``initial_adds`` = 1); the atomic forms add level by level, n_levels times."""
    a = np.asarray(abs_input_terms, dtype=np.float64)
    bound = (C_INPUT_TERM + n_levels) * U * a
    if initial is not None:
        bound = bound + initial_adds * U * (np.abs(np.asarray(initial, dtype=np.float64)) + a)
    return bound


def worst_fraction(err, bound):
    """largest err / bound over the elements with a positive bound (0 where there is none); elements with a zero
    bound must have zero error -- the caller asserts err <= bound everywhere"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    pos = bound > 0.0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
