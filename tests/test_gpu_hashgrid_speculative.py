"""The speculative hash backward (nerf_hash_encode_bwd_ws_store_spec / _tables_spec of csrc/hashgrid.hip: no count pass, every
bin sized from the record counts the PREVIOUS call left in the workspace) under estimates that do not fit the batch -- the same
batch, a batch that shrank, estimates from elsewhere, an overflow list that fills.  The contract, for any estimates a previous call
can have left:

  1  in bounds   nothing is written outside [workspace, workspace + workspace_bytes(n)) and the tables
  2  truthful    status[4] == 0 means d_table is complete; status[3] is exactly sum_bin max(true - capacity, 0); the counts left
                 for the next call are the batch's true ones, overflow included
  3  complete whenever it can be: estimates that exceed the record area are scaled down to it (status[6] == 1), the area always
                 holds the batch's own 8 L n records
  4  a complete call is within H.spec_overflow_bound of the fp64 sums (derived; nothing measured)
  5  a flagged call (status[4] == 1, the overflow list of 2^20 records was full) has status[3] > 2^20, entries nobody contributes to
                 exactly 0, every entry a partial sum of its own terms (|got| <= abs_sum + bound), everything finite
  E  after every speculative call the eight header words are zero and the host-mapped block equals the device block

Every call gets the view buf[:workspace_bytes(n)] of ONE buffer sized for the largest batch of the case (+ 1 MiB); what lies behind
the view is filled with a byte pattern before the speculative call and compared afterwards (statement 1).  The estimates sit at a
fixed offset in front of the workspace, so they survive the change of n.

The references are H.HashReference's exact corner lists; the float64 sums over them run on the device (index_add_)."""
import copy

import numpy as np
import pytest
import torch

import hashgrid_reference as H
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

# (n_levels, log2_hashmap_size, base_resolution, per_level_scale, bound), tables scattered to in one pass
SPEC_TABLES = {
    "instant_l16_t19": ((16, 19, 16, 1.5, 1.5), 1),        # 1,592 bins
    "deform_l12_t16": ((12, 16, 16, 1.5, 1.5), 3),         # 483 bins: Part 4's three deformation grids
}
VARIANTS = [("instant_l16_t19", False), ("deform_l12_t16", False), ("deform_l12_t16", True)]
VARIANT_IDS = ["instant_l16_t19", "deform_l12_t16-row_major", "deform_l12_t16-level_major"]
CANARY = 0xA5
SLACK = 1 << 20
MAX_OVERFLOW = 1 << 20          # kMaxOverflow
MAX_BINS = 65536                # kMaxBins


def record_capacity(n, virtual_levels):
    """bin_record_capacity: every corner of every point and level, + a quarter, + 64 per bin of the largest plan"""
    r = n * 8 * virtual_levels
    return r + r // 4 + 64 * MAX_BINS


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import ops as _ops
    return _ops


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ batches
def ray_points(n, seed):
    """samples along rays through the box, 16 per ray (the last ray cut where n is no multiple of 16): coherent like a training
    batch (runs of samples per coarse cell)"""
    g = torch.Generator().manual_seed(seed)
    rays = (n + 15) // 16
    o = torch.nn.functional.normalize(torch.randn(rays, 1, 3, generator=g), dim=-1) * 1.3
    d = torch.nn.functional.normalize(torch.randn(rays, 1, 3, generator=g), dim=-1)
    return (o * 0.3 + d * torch.linspace(-1.0, 1.0, 16).view(1, 16, 1)).reshape(-1, 3)[:n].contiguous().numpy()


def gradients(n, n_levels, k, seed, pattern="plain"):
    """d_feat fp32 [k, n, 2L]: every row non-zero ("plain"), every 7th row zero ("zero7"), row magnitudes 1e-6 .. 1e+6 ("span");
    the second and third tables as the three-table tests of test_gpu_hashgrid_edges.py derive them"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 2 * n_levels)).astype(np.float32)
    if pattern == "plain":
        d *= np.float32(1e-3)
    elif pattern == "zero7":
        d[::7] = 0.0
    else:
        assert pattern == "span"
        d = (d * 10.0 ** rng.uniform(-6.0, 6.0, size=(n, 1))).astype(np.float32)
    if k == 1:
        return d[None]
    assert k == 3
    return np.stack([d, -0.5 * d[::-1], d * rng.standard_normal((n, 1)).astype(np.float32)]).astype(np.float32)


class Batch:
    """points, gradients, the exact corner list, the per-bin record counts and (lazily, once) the float64 table gradients"""

    def __init__(self, rig, pts, d_feats, ref=None):
        self.rig, self.pts_h, self.d_h = rig, np.ascontiguousarray(pts, dtype=np.float32), d_feats
        self.n = self.pts_h.shape[0]
        self.ref = ref if ref is not None else H.HashReference(self.pts_h, rig.levels, rig.bound)
        self.bins = H.bin_counts(self.ref, d_feats)
        self.amax = float(np.abs(d_feats).max())
        self.pts, self.d = gpu(self.pts_h), gpu(d_feats)
        self._grads = None

    def subset(self, keep):
        ref = copy.copy(self.ref)
        ref.pts, ref.idx, ref.w, ref.frac = self.ref.pts[keep], self.ref.idx[keep], self.ref.w[keep], self.ref.frac[keep]
        ref.n = int(ref.pts.shape[0])
        return Batch(self.rig, self.pts_h[keep], np.ascontiguousarray(self.d_h[:, keep]), ref)

    def reference(self):
        """per table: (grad [E,2], count [E], abs_sum [E,2]) -- HashReference.table_gradient's sums, in float64 on the device"""
        if self._grads is None:
            E, L, n = self.rig.E, self.rig.L, self.n
            idx, w = gpu(self.ref.idx.reshape(-1)), gpu(self.ref.w)
            out = []
            for k in range(self.rig.k):
                g = self.d[k].double().view(n, L, 1, 2)
                contrib = (w[..., None] * g).reshape(-1, 2)
                grad = torch.zeros(E, 2, dtype=torch.float64, device="cuda").index_add_(0, idx, contrib)
                abs_sum = torch.zeros(E, 2, dtype=torch.float64, device="cuda").index_add_(0, idx, contrib.abs())
                live = (g != 0).any(dim=-1).expand(n, L, 8).reshape(-1)
                count = torch.bincount(idx[live], minlength=E)
                out.append((grad, count, abs_sum))
            self._grads = out
        return self._grads


class Rig:
    def __init__(self, ops, name):
        (L, log2_t, base, pls, bound), k = SPEC_TABLES[name]
        self.ops, self.lib, self.name, self.L, self.k, self.bound = ops, ops._lib.load(), name, L, k, bound
        self.levels = O.hash_grid_levels(L, log2_t, base, pls)
        self.t = ops.HashLevelTable(L, log2_t, base, pls)
        self.E = self.t.entries
        assert self.E == O.hash_grid_entries(self.levels)
        self.n_bins = k * sum(H.level_slices(self.levels))
        assert self.n_bins == {"instant_l16_t19": 1592, "deform_l12_t16": 483}[name]
        self.batches = {}

    def batch(self, key, make):
        if key not in self.batches:
            self.batches[key] = make()
        return self.batches[key]

    def rays(self, n, seed, pattern="plain"):
        return self.batch(("rays", n, seed, pattern), lambda: Batch(self, ray_points(n, seed), gradients(n, self.L, self.k, seed + 100, pattern)))

    def uniform(self, n, seed, pattern="plain"):
        return self.batch(("uniform", n, seed, pattern),
                          lambda: Batch(self, H.random_batch(self.bound, n, seed), gradients(n, self.L, self.k, seed + 100, pattern)))

    def workspace_bytes(self, n):
        if self.k == 1:
            return self.ops.hash_encode_bwd_workspace_bytes(n, self.L)
        return self.lib.nerf_hash_encode_bwd_tables_workspace_bytes(n, self.L, self.k)

    def capacity(self, n):
        return record_capacity(n, self.L * self.k)

    def buffer(self, n_largest):
        return torch.empty(self.workspace_bytes(n_largest) + SLACK, dtype=torch.uint8, device="cuda")

    # -- calls ---------------------------------------------------------------------------------------------------------------
    def counted(self, batch, buf):
        """the counted overwrite form on the view of the batch's own n: leaves the bins' true counts; returns d_table [k, E, 2]"""
        ws = buf[:self.workspace_bytes(batch.n)]
        out = torch.full((self.k, self.E, 2), float("nan"), device="cuda")
        if self.k == 1:
            self.ops.hash_encode_bwd(batch.pts, self.t, self.bound, batch.d[0], out[0], workspace=ws, overwrite=True)
        else:
            assert self.ops.hash_encode_bwd_tables(batch.pts, self.t, self.bound, [batch.d[i] for i in range(self.k)],
                                                   [out[i] for i in range(self.k)], lambda n_, L_, k_: ws)
        return out

    def speculative(self, batch, buf, begin, level_major=False):
        """one speculative call the way a producer and the engine drive it; checks statement 1 (the canary behind the view) and E
        (clean header, host block == device block); returns (status words, d_table [k, E, 2])"""
        ops, lib, n, VL = self.ops, self.lib, batch.n, self.L * self.k
        wb = self.workspace_bytes(n)
        ws, st = buf[:wb], torch.cuda.current_stream().cuda_stream
        if begin:
            ops._lib.check(lib.nerf_hash_encode_bwd_spec_begin(ws.data_ptr(), st), "spec_begin")
        # what the producer's backward leaves: fp32 bits of the largest |gradient|, and the level-major gradients
        # float2 [table * L + level][n]
        amax_p, lm_p = ops.hash_bwd_slots(ws, n, VL)
        a_off, l_off = amax_p - ws.data_ptr(), lm_p - ws.data_ptr()
        ws[a_off:a_off + 4].view(torch.float32).copy_(batch.d.abs().max().reshape(1))
        ws[l_off:l_off + n * VL * 8].view(torch.float32).view(VL, n, 2).copy_(
            torch.cat([batch.d[i] for i in range(self.k)], dim=1).view(n, VL, 2).permute(1, 0, 2))
        host = torch.full((8,), -1, dtype=torch.int32).pin_memory()
        out = torch.full((self.k, self.E, 2), float("nan"), device="cuda")
        buf[wb:].fill_(CANARY)
        if self.k == 1:
            ops._lib.check(lib.nerf_hash_encode_bwd_ws_store_spec(batch.pts.data_ptr(), n, self.L, *self.t.host_args(), float(self.bound),
                                                                  None if level_major else batch.d[0].data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                                  ws.numel(), host.data_ptr(), st), "store_spec")
        else:
            assert ops.hash_encode_bwd_tables(batch.pts, self.t, self.bound, [batch.d[i] for i in range(self.k)], [out[i] for i in range(self.k)],
                                              lambda n_, L_, k_: ws, spec_status=host, spec_lm=level_major)
        off = lib.nerf_hash_encode_bwd_spec_status(ws.data_ptr()) - ws.data_ptr()
        status = [v & 0xFFFFFFFF for v in ws[off:off + 32].view(torch.int32).cpu().tolist()]          # (synchronises)
        assert bool((buf[wb:] == CANARY).all()), f"{self.name}: the call wrote behind workspace_bytes({n})"
        assert [v & 0xFFFFFFFF for v in host.tolist()] == status, (host.tolist(), status)
        assert status[7] == 1
        assert ws[:32].view(torch.int32).cpu().tolist() == [0] * 8, "the call's last launch leaves the header clean"
        return status, out

    # -- checks --------------------------------------------------------------------------------------------------------------
    def check_complete(self, tag, batch, out):
        """statement 4, and entries nobody contributes to are exactly 0; prints the fraction of the bound used"""
        worst = 0.0
        for k, (grad, count, abs_sum) in enumerate(batch.reference()):
            bound = gpu(H.spec_overflow_bound(count.cpu().numpy(), abs_sum.cpu().numpy(), batch.amax, batch.n))
            err = (out[k].double() - grad).abs()
            bad = ~(err <= bound)                                            # NaN: an entry the call did not store
            worst = max(worst, float(torch.where(bound > 0, err / bound, torch.zeros_like(err)).nan_to_num(nan=float("inf")).max()))
            assert not bool(bad.any()), f"{tag} table {k}: {int(bad.sum())} elements beyond the bound, worst {worst:.3f} x"
            assert bool((out[k][count == 0] == 0).all()), f"{tag} table {k}: an entry without a contribution is not 0"
        print(f"[headroom] {tag}: {worst:.4f} of the bound")

    def check_flagged(self, tag, batch, out):
        """statement 5: finite, exact zeros where nothing contributes, |got| <= abs_sum + bound"""
        assert bool(torch.isfinite(out).all()), f"{tag}: not finite"
        for k, (grad, count, abs_sum) in enumerate(batch.reference()):
            bound = gpu(H.spec_overflow_bound(count.cpu().numpy(), abs_sum.cpu().numpy(), batch.amax, batch.n))
            assert bool((out[k][count == 0] == 0).all()), f"{tag} table {k}: an entry without a contribution is not 0"
            bad = out[k].double().abs() > abs_sum + bound
            assert not bool(bad.any()), f"{tag} table {k}: {int(bad.sum())} entries larger than the sum of their own terms"


_RIGS = {}


def rig_of(ops, name):
    if name not in _RIGS:
        _RIGS[name] = Rig(ops, name)
    return _RIGS[name]


def overflow_of(true_bins, capacities):
    return int(np.maximum(np.asarray(true_bins, dtype=np.int64) - np.asarray(capacities, dtype=np.int64), 0).sum())


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name,level_major", VARIANTS, ids=VARIANT_IDS)
def test_same_batch_without_cut_bins_is_bit_equal_to_the_counted_form(ops, name, level_major):
    """A: a uniform batch of 4,000 points whose bins all stay below the 32,768 records at which a bin is cut (count AND capacity:
    29,000 + 29,000 / 8 + 64 < 32,768): every entry is one integer sum converted once at the same power-of-two scale in both forms,
    so the speculative result equals the counted one bit for bit, after a counted call and after itself.  Level 0 is ONE bin (4,096
    entries) that takes eight records of every live point, so 4,000 live points would put 32,000 records into it: every 7th
    gradient row is zero here (3,428 live rows, 27,424 records in that bin), which keeps the batch size and the 29,000."""
    rig = rig_of(ops, name)
    batch = rig.uniform(4000, 17, "zero7")
    assert int(batch.bins.max()) <= 29000
    planned = int(H.planned_capacities(batch.bins).sum())
    buf = rig.buffer(batch.n)
    want = rig.counted(batch, buf)
    for round_, begin in (("after a counted call", True), ("after a speculative call", False)):
        status, out = rig.speculative(batch, buf, begin, level_major)
        assert status[3] == 0 and status[4] == 0 and status[6] == 0, (round_, status)
        assert status[1] == planned and status[5] == planned, (round_, status, planned)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), f"{name} {round_}: not bit-equal to the counted form"
    rig.check_complete(f"A {name} speculative == counted", batch, out)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("name,level_major", VARIANTS, ids=VARIANT_IDS)
def test_shrunk_batch_whose_plan_does_not_fit_is_scaled_and_complete(ops, name, level_major):
    """B: estimates of a batch, then its subset index % 5 < 3 (0.6 of it: inside the engine's window of 0.5 .. 1.1): est + est / 8 + 64
    summed over the bins exceeds the record area of the smaller n.  The plan pass scales the capacities down to the area
    (status[6] == 1, status[1] <= capacity) and the call is complete; the same batch again, now on its own counts, is not scaled,
    overflows nothing and plans exactly from the small batch's true counts -- the scaled call left them."""
    rig = rig_of(ops, name)
    n_big = 96000 if rig.k == 1 else 48000
    big = rig.rays(n_big, 1)
    small = rig.batch(("subset", n_big), lambda: big.subset(np.arange(n_big) % 5 < 3))
    assert small.n == n_big * 3 // 5 and int(small.bins.sum()) == 8 * small.n * rig.L * rig.k        # every gradient row is non-zero
    capacity = rig.capacity(small.n)
    assert capacity == (13410304 if rig.k == 1 else 14562304)
    planned_big = int(H.planned_capacities(big.bins).sum())
    assert planned_big > capacity and planned_big >= (13920000 if rig.k == 1 else 15580000), (planned_big, capacity)
    buf = rig.buffer(big.n)
    rig.counted(big, buf)
    status, out = rig.speculative(small, buf, True, level_major)
    print(f"B {name}: planned {planned_big} > capacity {capacity}; scaled plan {status[1]}, {status[3]} records overflowed, status {status}")
    assert status[6] == 1 and status[4] == 0 and status[1] <= capacity, status
    room = capacity - 64 * rig.n_bins
    scaled = big.bins * room // int((big.bins + (big.bins >> 3)).sum()) + 64
    assert status[1] == int(scaled.sum()) and status[3] == overflow_of(small.bins, scaled), (status, int(scaled.sum()))
    rig.check_complete(f"B {name} shrunk batch, scaled plan", small, out)
    status, out = rig.speculative(small, buf, False, level_major)
    assert status[6] == 0 and status[3] == 0 and status[4] == 0, status
    assert status[1] == int(H.planned_capacities(small.bins).sum()), status
    rig.check_complete(f"B {name} the same batch on the counts the scaled call left", small, out)


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("name,level_major", VARIANTS, ids=VARIANT_IDS)
def test_estimates_from_elsewhere_overflow_into_the_list(ops, name, level_major):
    """C: estimates of a 16-point batch, then a batch whose records (768,000 and 864,000: below 2^20) all fit the overflow list:
    complete, status[3] exact, within the bound that charges every record two more roundings; with every 7th gradient row zero, and
    with row magnitudes from 1e-6 to 1e+6."""
    rig = rig_of(ops, name)
    n = 6000 if rig.k == 1 else 3000
    assert 8 * n * rig.L * rig.k < MAX_OVERFLOW
    tiny = rig.rays(16, 5)
    buf = rig.buffer(n)
    for pattern in ("zero7", "span"):
        batch = rig.rays(n, 2, pattern)
        rig.counted(tiny, buf)
        status, out = rig.speculative(batch, buf, True, level_major)
        want = overflow_of(batch.bins, H.planned_capacities(tiny.bins))
        print(f"C {name} {pattern}: {status[3]} of {int(batch.bins.sum())} records overflowed, status {status}")
        assert status[4] == 0 and status[6] == 0, status
        assert status[3] == want and want > int(batch.bins.sum()) // 2, (status, want)
        rig.check_complete(f"C {name} {pattern} estimates of 16 points", batch, out)


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("name,level_major", VARIANTS, ids=VARIANT_IDS)
def test_full_overflow_list_is_flagged_and_leaves_partial_sums(ops, name, level_major):
    """D: estimates of the 16-point batch, then 1,536,000 (1,728,000) records against bins that hold 0.11 M at most: the list of 2^20
    fills, the call says so (status[4] == 1, status[3] > 2^20 and still exact) and what it stored is defined; it still left the
    batch's true counts, so the next speculative call on the batch is complete."""
    rig = rig_of(ops, name)
    n = 12000 if rig.k == 1 else 6000
    tiny, batch = rig.rays(16, 5), rig.rays(n, 3)
    capacities = H.planned_capacities(tiny.bins)
    assert int(capacities.sum()) <= 110000 and int(batch.bins.sum()) - int(capacities.sum()) > MAX_OVERFLOW
    buf = rig.buffer(n)
    rig.counted(tiny, buf)
    status, out = rig.speculative(batch, buf, True, level_major)
    print(f"D {name}: {status[3]} of {int(batch.bins.sum())} records overflowed, status {status}")
    assert status[4] == 1 and status[7] == 1 and status[3] > MAX_OVERFLOW, status
    assert status[3] == overflow_of(batch.bins, capacities), status
    rig.check_flagged(f"D {name} overflow list full", batch, out)
    status, out = rig.speculative(batch, buf, False, level_major)
    assert status[4] == 0 and status[3] == 0 and status[6] == 0, status
    assert status[1] == int(H.planned_capacities(batch.bins).sum()), status
    rig.check_complete(f"D {name} the same batch on the counts the flagged call left", batch, out)
