"""Every entry point of csrc/hashgrid.hip against the exact fp64 corner-list reference (tests/hashgrid_reference.py)
at the probe points, level tables and batches named there.  Every tolerance is a bound function of the helper, evaluated
on reference-side quantities; each test prints the largest fraction of its bound the kernel used ("[headroom] ...").

The consumers of the operand image never use the columns the forward leaves unwritten: the Part 4 deformation chain
(12 levels, 24 of 32 columns) loads them but selects 0 for every feature >= kHashDeform (p4mlp.hip, the tri-grid blend:
``valid = 16 ks + 8 half + j < kHashDeform``), its weight-gradient job reads the blended stash with nat_valid =
kHashDeform, and the Instant decoder's image has 16 levels = 32 written columns.  So the image tests assert the written
map and nothing about the unwritten words."""
import ctypes

import numpy as np
import pytest
import torch

import hashgrid_reference as H
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

TABLES = list(H.LEVEL_TABLES)
POISON = 0x7B7B                 # a finite bf16 (1.3e36) and fp16 (61280) bit pattern
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import ops as _ops
    return _ops


_CASES = {}


def case_of(ops, name):
    """levels, table and probe points of one LEVEL_TABLES entry, with the references every test of the table shares"""
    if name in _CASES:
        return _CASES[name]
    n_levels, log2_t, base, pls, bound = H.LEVEL_TABLES[name]
    levels = O.hash_grid_levels(n_levels, log2_t, base, pls)
    t = ops.HashLevelTable(n_levels, log2_t, base, pls)
    assert t.entries == O.hash_grid_entries(levels)
    rng = np.random.default_rng(5)
    table = (rng.random((t.entries, 2)) - 0.5).astype(np.float32)
    table_h = torch.from_numpy(table).half()
    c = dict(name=name, levels=levels, t=t, bound=bound, L=n_levels, table=table, table_gpu=torch.from_numpy(table).cuda(),
             table_h_gpu=table_h.cuda(), table_h64=table_h.double().numpy(), probes=H.probe_points(levels, bound, seed=0), batches={})
    _CASES[name] = c
    return c


def batch_of(c, which):
    """(pts fp32 [n,3], d_feat fp32 [n,2L], HashReference) of a named batch, built once"""
    if which in c["batches"]:
        return c["batches"][which]
    rng = np.random.default_rng({"probe": 1, "one_cell": 2, "zero7": 3, "span": 4}[which])
    if which == "probe":
        pts = c["probes"]
    elif which == "one_cell":
        pts = H.one_cell_batch(c["bound"])
    else:
        pts = H.random_batch(c["bound"], 2000, 17)
    d_feat = rng.standard_normal((pts.shape[0], 2 * c["L"])).astype(np.float32)
    if which == "zero7":
        d_feat[::7] = 0.0                                            # rows the kernels skip
    if which == "span":                                              # magnitudes from 1e-6 to 1e+6, row by row
        d_feat = (d_feat * 10.0 ** rng.uniform(-6.0, 6.0, size=(pts.shape[0], 1))).astype(np.float32)
    ref = H.HashReference(pts, c["levels"], c["bound"])
    c["batches"][which] = (pts, d_feat, ref)
    return c["batches"][which]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(tag, got, want, bound):
    """|got - want| <= bound elementwise (float64 on the device for the table-sized arrays); prints the fraction used"""
    got = got.double() if isinstance(got, torch.Tensor) else gpu(np.asarray(got, dtype=np.float64))
    want, bound = gpu(np.asarray(want, dtype=np.float64)), gpu(np.asarray(bound, dtype=np.float64))
    err = (got.to(want.device) - want).abs()
    frac = float(torch.where(bound > 0, err / bound, torch.zeros_like(err)).max())
    print(f"[headroom] {tag}: {frac:.4f} of the bound")
    bad = err > bound
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} elements beyond the bound, worst {frac:.3f} x"
    return frac


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", TABLES)
def test_forward_indices_and_features(ops, name):
    c = case_of(ops, name)
    pts, _, ref = batch_of(c, "probe")
    feat, idx = ops.hash_encode_fwd(gpu(pts), c["table_gpu"], c["t"], c["bound"], want_index=True)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ref.idx)
    want = ref.features(c["table"].astype(np.float64))
    check(f"forward fp32 table {name}", feat, want, H.forward_bound(ref.abs_terms))
    feat_h, _ = ops.hash_encode_fwd(gpu(pts), c["table_h_gpu"], c["t"], c["bound"])
    want_h = ref.features(c["table_h64"])
    check(f"forward fp16 table {name}", feat_h, want_h, H.forward_bound(ref.abs_terms))
    # the same arithmetic after an exact conversion: bit for bit
    feat_hf, _ = ops.hash_encode_fwd(gpu(pts), c["table_h_gpu"].float(), c["t"], c["bound"])
    assert torch.equal(feat_h.view(torch.int32), feat_hf.view(torch.int32))
    # one cell holds every point, and the upper corner of the box: the wrap of the dense levels
    pts1, _, ref1 = batch_of(c, "one_cell")
    feat1, idx1 = ops.hash_encode_fwd(gpu(pts1), c["table_gpu"], c["t"], c["bound"], want_index=True)
    assert np.array_equal(idx1.cpu().numpy().astype(np.int64), ref1.idx)
    check(f"forward fp32 table, one cell {name}", feat1, ref1.features(c["table"].astype(np.float64)), H.forward_bound(ref1.abs_terms))


def image_words(n, L):
    return H.nat_padded_rows(n) * 16 * ((2 * L + 15) // 16)


@pytest.mark.parametrize("fp16_image", [False, True], ids=["bf16_image", "fp16_image"])
@pytest.mark.parametrize("fp16_table", [False, True], ids=["fp32_table", "fp16_table"])
@pytest.mark.parametrize("name", TABLES)
def test_operand_image_decodes_to_the_rounded_features(ops, name, fp16_table, fp16_image):
    c = case_of(ops, name)
    probes, L = c["probes"], c["L"]
    table = c["table_h_gpu"] if fp16_table else c["table_gpu"]
    for n in H.ROW_COUNTS + (probes.shape[0],):
        pts = gpu(probes[:n])
        feat, _ = ops.hash_encode_fwd(pts, table, c["t"], c["bound"])
        words = image_words(n, L)
        image = torch.full((words + 64,), POISON, dtype=torch.int16, device="cuda")          # 64 guard words behind the image
        ops.hash_encode_fwd_nat(pts, table, c["t"], c["bound"], image, fp16=fp16_image)
        raw = image.cpu().numpy().view(np.uint16)
        assert np.all(raw[words:] == POISON), "the forward wrote behind the padded image"
        changed = raw[:words] != POISON
        assert np.array_equal(changed, H.nat_written_words(n, L)), f"n={n}: written words differ from the map"
        rows = H.nat_rows(raw, n, L)
        f = feat.cpu().numpy()
        expect = H.round_to_f16_words(f) if fp16_image else H.round_to_bf16_words(f)
        assert np.array_equal(rows[:n, :2 * L], expect), f"n={n}: image rows are not the round-to-nearest-even cast of the features"
        assert np.all(rows[n:, :2 * L] == rows[n - 1, :2 * L]), f"n={n}: pad rows do not repeat row n-1"
        values, written = H.decode_nat(raw, n, L, "fp16" if fp16_image else "bf16")
        assert np.all(np.isfinite(values[written]))


@pytest.mark.parametrize("fp16_image", [False, True], ids=["bf16_image", "fp16_image"])
@pytest.mark.parametrize("name", TABLES)
def test_operand_images_of_three_tables_equal_three_single_launches(ops, name, fp16_image):
    c = case_of(ops, name)
    probes, L, E = c["probes"], c["L"], c["t"].entries
    rng = np.random.default_rng(9)
    tabs = torch.from_numpy((rng.random((3 * E, 2)) - 0.5).astype(np.float32)).half().cuda()
    for n in (33, probes.shape[0]):
        pts, words = gpu(probes[:n]), image_words(n, L)
        img = torch.full((3, words), POISON, dtype=torch.int16, device="cuda")
        assert ops.hash_encode_fwd_nat_tables(pts, [tabs[k * E:(k + 1) * E] for k in range(3)], c["t"], c["bound"], [img[k] for k in range(3)],
                                              fp16=fp16_image)
        for k in range(3):
            one = torch.full((words,), POISON, dtype=torch.int16, device="cuda")
            ops.hash_encode_fwd_nat(pts, tabs[k * E:(k + 1) * E], c["t"], c["bound"], one, fp16=fp16_image)
            assert torch.equal(img[k], one)
            feat, _ = ops.hash_encode_fwd(pts, tabs[k * E:(k + 1) * E], c["t"], c["bound"])
            rows = H.nat_rows(one.cpu().numpy().view(np.uint16), n, L)
            f = feat.cpu().numpy()
            assert np.array_equal(rows[:n, :2 * L], H.round_to_f16_words(f) if fp16_image else H.round_to_bf16_words(f))


# ------------------------------------------------------------------------------------------------ table gradient
BATCHES = ("probe", "one_cell", "zero7", "span")


def workspace(ops, n, L):
    return torch.empty(max(ops.hash_encode_bwd_workspace_bytes(n, L), 256), dtype=torch.uint8, device="cuda")


def table_reference(c, which):
    pts, d_feat, ref = batch_of(c, which)
    key = ("table_gradient", which)
    if key not in c:
        c[key] = ref.table_gradient(d_feat.astype(np.float64))
    grad, count, abs_sum = c[key]
    return pts, d_feat, ref, grad, count, abs_sum


def producer_slots(ops, lib, ws, n, L, d_feat):
    """what a decoder's backward leaves in the workspace for the forms that do not count: the fp32 bits of the largest
    |gradient| and the level-major gradients"""
    amax_p, lm_p = ctypes.c_void_p(), ctypes.c_void_p()
    ops._lib.check(lib.nerf_hash_encode_bwd_ws_slots(ws.data_ptr(), n, L, ctypes.byref(amax_p), ctypes.byref(lm_p)), "slots")
    a_off, l_off = amax_p.value - ws.data_ptr(), lm_p.value - ws.data_ptr()
    ws[a_off:a_off + 4].view(torch.float32).copy_(d_feat.abs().max().reshape(1))
    ws[l_off:l_off + n * L * 8].view(torch.float32).view(L, n, 2).copy_(d_feat.view(n, L, 2).permute(1, 0, 2))


def spec_call(ops, lib, c, pts, d_feat, out, ws, begin):
    n, L, st = pts.shape[0], c["L"], torch.cuda.current_stream().cuda_stream
    if begin:
        ops._lib.check(lib.nerf_hash_encode_bwd_spec_begin(ws.data_ptr(), st), "spec_begin")
    producer_slots(ops, lib, ws, n, L, d_feat)
    host = torch.full((8,), -1, dtype=torch.int32).pin_memory()
    ops._lib.check(lib.nerf_hash_encode_bwd_ws_store_spec(pts.data_ptr(), n, L, *c["t"].host_args(), float(c["bound"]), d_feat.data_ptr(),
                                                          out.data_ptr(), ws.data_ptr(), ws.numel(), host.data_ptr(), st), "store_spec")
    off = lib.nerf_hash_encode_bwd_spec_status(ws.data_ptr()) - ws.data_ptr()
    status = ws[off:off + 32].view(torch.int32).cpu().tolist()
    assert host.tolist() == status
    return status


FORMS = ("atomic", "levels", "ws_accumulate", "ws_store", "precounted", "speculative", "deterministic")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TABLES)
def test_table_gradient_forms(ops, name, form):
    """Each form on the probe set, the one-cell batch (5000 points: bins cut into several items), a batch with every
    7th gradient row zero and a batch whose gradient rows span 1e-6 .. 1e+6.  On the last one the fixed-point forms'
    bound is count * step with the step set by the LAUNCH's largest |d_feat|: an entry fed only by small rows may
    come out as 0 -- that is the format's resolution, and the bound says so instead of hiding it."""
    c = case_of(ops, name)
    lib = ops._lib.load()
    t, L, E, b = c["t"], c["L"], c["t"].entries, c["bound"]
    for which in BATCHES:
        pts_h, d_feat_h, ref, grad, count, abs_sum = table_reference(c, which)
        n, amax = pts_h.shape[0], float(np.abs(d_feat_h).max())
        pts, d_feat = gpu(pts_h), gpu(d_feat_h)
        tag = f"table gradient {form} {name} {which}"
        float_bound = lambda init=None: H.scatter_float_bound(count, abs_sum, n, init)
        fixed_bound = lambda init=None: H.scatter_fixed_bound(count, abs_sum, amax, n, init)
        if form == "atomic":
            out = torch.zeros(E, 2, device="cuda")
            ops.hash_encode_bwd(pts, t, b, d_feat, out)
            check(tag, out, grad, float_bound())
        elif form == "levels":
            out = torch.zeros(E, 2, device="cuda")
            cuts = sorted({0, L // 3, (2 * L) // 3, L})
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                ops.hash_encode_bwd(pts, t, b, d_feat, out, level_range=(lo, hi))
            check(tag, out, grad, float_bound())
        elif form == "ws_accumulate":
            init_h = (np.random.default_rng(8).standard_normal((E, 2)) * 0.01).astype(np.float32)
            out = gpu(init_h)
            ops.hash_encode_bwd(pts, t, b, d_feat, out, workspace=workspace(ops, n, L))
            check(tag, out.double() - gpu(init_h).double(), grad, fixed_bound(init_h))
            assert torch.equal(out[gpu(count == 0)], gpu(init_h)[gpu(count == 0)])              # untouched entries: not even rewritten
        elif form == "ws_store":
            ws = workspace(ops, n, L)
            out = torch.full((E, 2), SENTINEL, device="cuda")
            ops.hash_encode_bwd(pts, t, b, d_feat, out, workspace=ws, overwrite=True)
            check(tag, out, grad, fixed_bound())                                                # entries without a contribution: exactly 0
            lo, hi = (L // 2, L) if L > 1 else (0, 1)
            part = torch.full((E, 2), SENTINEL, device="cuda")
            ops.hash_encode_bwd(pts, t, b, d_feat, part, level_range=(lo, hi), workspace=ws, overwrite=True)
            e0, e1 = int(t.offset[lo]), int(t.offset[hi - 1] + t.size[hi - 1])
            assert bool((part[:e0] == SENTINEL).all()) and bool((part[e1:] == SENTINEL).all())
            check(tag + " (upper levels)", part[e0:e1], grad[e0:e1], fixed_bound()[e0:e1])
        elif form == "precounted":
            ws = workspace(ops, n, L)
            st = torch.cuda.current_stream().cuda_stream
            image = torch.empty(image_words(n, L), dtype=torch.int16, device="cuda")
            ops._lib.check(lib.nerf_hash_encode_fwd_f16_hist(pts.data_ptr(), n, c["table_h_gpu"].data_ptr(), L, *t.host_args(), float(b),
                                                             image.data_ptr(), ws.data_ptr(), ws.numel(), st), "fwd_f16_hist")
            producer_slots(ops, lib, ws, n, L, d_feat)
            out = torch.full((E, 2), SENTINEL, device="cuda")
            ops._lib.check(lib.nerf_hash_encode_bwd_ws_store_precounted(pts.data_ptr(), n, L, *t.host_args(), float(b), out.data_ptr(),
                                                                        ws.data_ptr(), ws.numel(), st), "precounted")
            check(tag, out, grad, fixed_bound())
        elif form == "speculative":
            ws = workspace(ops, n, L)
            tmp = torch.empty(E, 2, device="cuda")
            ops.hash_encode_bwd(pts, t, b, d_feat, tmp, workspace=ws, overwrite=True)           # counted: leaves the bins' true counts
            for round_, begin in (("after a counted call", True), ("after a speculative call", False)):
                out = torch.full((E, 2), SENTINEL, device="cuda")
                status = spec_call(ops, lib, c, pts, d_feat, out, ws, begin)
                assert status[3] == 0, f"{tag} {round_}: {status[3]} records overflowed bins sized from the same batch"
                assert status[4] == 0, f"{tag} {round_}: records lost ({status[4]})"
                check(f"{tag} {round_}", out, grad, fixed_bound())
        else:
            assert form == "deterministic"
            ops.set_deterministic(True)
            try:
                ws = workspace(ops, n, L)
                runs = []
                for _ in range(2):
                    out = torch.full((E, 2), SENTINEL, device="cuda")
                    ops.hash_encode_bwd(pts, t, b, d_feat, out, workspace=ws, overwrite=True)
                    runs.append(out)
                assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
                check(tag + " store", runs[0], grad, fixed_bound())
                acc = [torch.zeros(E, 2, device="cuda") for _ in range(2)]
                for a in acc:
                    ops.hash_encode_bwd(pts, t, b, d_feat, a)                                   # the wrapper gives it a workspace
                assert torch.equal(acc[0].view(torch.int32), acc[1].view(torch.int32))
                check(tag + " accumulate", acc[0], grad, fixed_bound(np.zeros((E, 2))))
            finally:
                ops.set_deterministic(False)


def three_tables(c, which):
    """(pts, d_feats fp32 [3, n, 2L], their largest magnitude, [(grad, count, abs_sum)] per table) of a named batch, built once:
    one header, one scale for the whole launch"""
    key = ("three_tables", which)
    if key not in c:
        pts_h, d_feat_h, ref = batch_of(c, which)
        n = pts_h.shape[0]
        rng = np.random.default_rng(21)
        d_feats_h = np.stack([d_feat_h, -0.5 * d_feat_h[::-1], d_feat_h * rng.standard_normal((n, 1)).astype(np.float32)]).astype(np.float32)
        c[key] = (pts_h, d_feats_h, float(np.abs(d_feats_h).max()), [ref.table_gradient(d_feats_h[k].astype(np.float64)) for k in range(3)])
    return c[key]


def tables_workspace(lib, n, L, k):
    return torch.empty(max(lib.nerf_hash_encode_bwd_tables_workspace_bytes(n, L, k), 256), dtype=torch.uint8, device="cuda")


def check_three_tables(tag, flat, refs, amax, n):
    for k, (grad, count, abs_sum) in enumerate(refs):
        check(f"{tag} table {k}", flat[k], grad, H.scatter_fixed_bound(count, abs_sum, amax, n))


@pytest.mark.parametrize("name", TABLES)
def test_table_gradient_of_three_tables_in_one_pass(ops, name):
    c = case_of(ops, name)
    lib = ops._lib.load()
    t, L, E, b = c["t"], c["L"], c["t"].entries, c["bound"]
    for which in BATCHES:
        pts_h, d_feats_h, amax, refs = three_tables(c, which)
        n = pts_h.shape[0]
        flat = torch.full((3, E, 2), SENTINEL, device="cuda")
        d_feats = gpu(d_feats_h)
        ws_of = lambda n_, L_, k_: tables_workspace(lib, n_, L_, k_)
        assert ops.hash_encode_bwd_tables(gpu(pts_h), t, b, [d_feats[k] for k in range(3)], [flat[k] for k in range(3)], ws_of)
        check_three_tables(f"table gradient ws_store_tables {name} {which}", flat, refs, amax, n)


@pytest.mark.parametrize("level_major", [False, True], ids=["row_major", "level_major"])
@pytest.mark.parametrize("name", TABLES)
def test_table_gradient_of_three_tables_speculative(ops, name, level_major):
    """nerf_hash_encode_bwd_ws_store_tables_spec after a counted call on the same workspace, then after itself; the gradients
    row-major, or (d_feat NULL) as the level-major copy a producer leaves in the workspace: float2 [table * L + level][n], the
    row hash_bin_scatter_kernel reads as grad_lm[blockIdx.y * n + p] and nerf_p4_deform_bwd writes"""
    c = case_of(ops, name)
    lib = ops._lib.load()
    t, L, E, b = c["t"], c["L"], c["t"].entries, c["bound"]
    for which in BATCHES:
        pts_h, d_feats_h, amax, refs = three_tables(c, which)
        n = pts_h.shape[0]
        pts, d_feats = gpu(pts_h), gpu(d_feats_h)
        ws = tables_workspace(lib, n, L, 3)
        ws_of = lambda n_, L_, k_: ws
        tmp = torch.empty(3, E, 2, device="cuda")
        assert ops.hash_encode_bwd_tables(pts, t, b, [d_feats[k] for k in range(3)], [tmp[k] for k in range(3)], ws_of)      # counted: leaves the true counts
        off = lib.nerf_hash_encode_bwd_spec_status(ws.data_ptr()) - ws.data_ptr()
        for round_, begin in (("after a counted call", True), ("after a speculative call", False)):
            tag = f"table gradient ws_store_tables_spec {'level-major' if level_major else 'row-major'} {name} {which} {round_}"
            if begin:
                ops._lib.check(lib.nerf_hash_encode_bwd_spec_begin(ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "spec_begin")
            producer_slots(ops, lib, ws, n, 3 * L, torch.cat([d_feats[k] for k in range(3)], dim=1))
            host = torch.full((8,), -1, dtype=torch.int32).pin_memory()
            flat = torch.full((3, E, 2), SENTINEL, device="cuda")
            assert ops.hash_encode_bwd_tables(pts, t, b, [d_feats[k] for k in range(3)], [flat[k] for k in range(3)], ws_of, spec_status=host,
                                              spec_lm=level_major)
            status = ws[off:off + 32].view(torch.int32).cpu().tolist()
            assert host.tolist() == status
            assert status[3] == 0, f"{tag}: {status[3]} records overflowed bins sized from the same batch"
            assert status[4] == 0, f"{tag}: records lost ({status[4]})"
            check_three_tables(tag, flat, refs, amax, n)


@pytest.mark.parametrize("name", TABLES)
def test_table_gradient_of_three_tables_deterministic(ops, name):
    c = case_of(ops, name)
    lib = ops._lib.load()
    t, L, E, b = c["t"], c["L"], c["t"].entries, c["bound"]
    ops.set_deterministic(True)
    try:
        for which in BATCHES:
            pts_h, d_feats_h, amax, refs = three_tables(c, which)
            n = pts_h.shape[0]
            pts, d_feats = gpu(pts_h), gpu(d_feats_h)
            ws = tables_workspace(lib, n, L, 3)
            runs = []
            for _ in range(2):
                flat = torch.full((3, E, 2), SENTINEL, device="cuda")
                assert ops.hash_encode_bwd_tables(pts, t, b, [d_feats[k] for k in range(3)], [flat[k] for k in range(3)], lambda n_, L_, k_: ws)
                runs.append(flat)
            assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
            check_three_tables(f"table gradient ws_store_tables deterministic {name} {which}", runs[0], refs, amax, n)
    finally:
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ input gradient
INPUT_FORMS = ("fp32", "fp16", "accumulate", "level_major", "level_major_accumulate", "ordered_fp32", "ordered_fp16", "ordered_accumulate")


@pytest.mark.parametrize("form", INPUT_FORMS)
@pytest.mark.parametrize("name", TABLES)
def test_input_gradient_forms(ops, name, form):
    c = case_of(ops, name)
    t, L, b = c["t"], c["L"], c["bound"]
    for which in ("probe", "zero7", "span"):
        pts_h, d_feat_h, ref = batch_of(c, which)
        n = pts_h.shape[0]
        pts, d_feat = gpu(pts_h), gpu(d_feat_h)
        fp32_table = form in ("fp32", "ordered_fp32")
        table = c["table_gpu"] if fp32_table else c["table_h_gpu"]
        want = ref.input_gradient(c["table"].astype(np.float64) if fp32_table else c["table_h64"], d_feat_h.astype(np.float64))
        init_h = None
        ordered = form.startswith("ordered")
        if ordered:
            ops.set_deterministic(True)
        try:
            if form in ("fp32", "fp16", "ordered_fp32", "ordered_fp16"):
                out = ops.hash_encode_bwd_input(pts, table, t, b, d_feat)
            elif form in ("accumulate", "ordered_accumulate"):
                init_h = np.random.default_rng(6).standard_normal((n, 3)).astype(np.float32)
                out = ops.hash_encode_bwd_input(pts, table, t, b, d_feat, add_to=gpu(init_h))
            else:
                lm = d_feat.view(n, L, 2).permute(1, 0, 2).contiguous()
                add_to = None
                if form == "level_major_accumulate":
                    init_h = np.random.default_rng(6).standard_normal((n, 3)).astype(np.float32)
                    add_to = gpu(init_h)
                out = ops.hash_encode_bwd_input(pts, table, t, b, None, add_to=add_to, grad_lm=lm.data_ptr())
            torch.cuda.synchronize()
        finally:
            if ordered:
                ops.set_deterministic(False)
        got = out.double().cpu().numpy()
        if init_h is not None:
            got = got - init_h.astype(np.float64)
        # accumulate: the ordered kernel adds its register sum to the initial value once, the atomic kernel once per level
        bound = H.input_gradient_bound(ref.abs_input_terms, L, init_h, initial_adds=1 if ordered else L)
        check(f"input gradient {form} {name} {which}", got, want, bound)
        if init_h is None:
            assert np.all(got[~ref.inside] == 0.0)                   # strictly outside on an axis: exactly 0.0
        else:
            assert np.array_equal(out.cpu().numpy()[~ref.inside], init_h[~ref.inside])
        if which == "probe":
            raw = H.normalise_f32(pts_h, b)
            face = (raw == 0.0) | (raw == 1.0)                       # exactly +-bound (and the float next to +bound, which rounds onto it)
            assert face.sum() >= 15
            # the reference's value there is not zero, and an open interval (gradient 0) would miss it by more than the bound
            assert float((np.abs(want[face]) > bound[face]).mean()) > 0.9
            nodes = (ref.frac == 0.0).any(axis=1)                    # a coordinate on a lattice node of some level: one-sided value of floor's cell
            assert nodes.any()
