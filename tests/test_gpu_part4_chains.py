"""The two Part 4 chains (csrc/p4mlp.hip), one chain at a time, against the matched float64 chain of tests/part4_reference.py
(pytest -m gpu; one MI355X).

The field is cut at the hash features: the C entries nerf_p4_pack, nerf_p4_deform_fwd / _bwd and nerf_p4_canon_fwd / _bwd are driven
directly, on feature images written by ops.hash_encode_fwd_nat(..., fp16=True) into part4.Workspace's public slots; the reference
takes ops.hash_encode_fwd's fp32 features and rounds them to fp16 itself (tests/test_gpu_instant_shapes.py::reference's move; the
hash kernels are pinned exactly by tests/test_gpu_hashgrid_edges.py).  No hash cell is crossed, so nothing amplifies a rounding and
the bounds are those of the chains' own arithmetic.  The canonical chain is fed features at arbitrary points, not at x_c.

Bounds.  Per quantity max(floor, 4 x yardstick) (part4_reference.bounds): the yardstick is the matched chain with float32 sums
against itself with float64 sums on these inputs -- no kernel involved -- pooled over the cases and over four float32 summation
orders defined in part4_reference._mm (why pooled: part4_reference.yardsticks);
floors 2^-9 (bf16-rounded gradients), 2^-11 (fp16-rounded forward outputs), 1e-6 (d_feat, displacement_scale: summed in fp32);
tests/test_part4_reference.py asserts the caps (2e-3 forward, 2e-2 gradients) on the CPU.  Quantities: dx relative to max |dx|, rgb
max-abs, sigma relative L2; each of the 13 parameter blocks, each input block of D1 [hash 24 | tm 64], S1 [hash 32 | tcode 21] and
C1 [h16 16 | dir 27], and each d_feat, relative L2.  Every test prints its figures next to the bound (pytest -s, lines starting with FIG).

Inputs (part4_reference.chain_inputs): one draw of 1,025 rows, a case takes the first n; the golden g14 network weights, and one
random draw over the whole flat vector with the pads filled (the displacement head D3 made one-signed: with zero-mean rows dx is a
difference of terms larger than itself, and one fp16 unit of one activation is then more than 5e-4 of max |dx|, a quarter of the cap);
displacement_scale 0.1; non-zero-mean upstream gradients; t in [0, 1] with 0, 0.5, 1, the fp32 neighbours of 0.5 and 0.25 planted.

Observed
--------
One MI355X; this file: 54 tests in 4.7 s.  Yardstick (CPU, largest over the cases and the float32 orders), bound, largest figure over
the cases and where.
quantity    yardstick  bound     largest GPU figure (fraction of the bound; case)
dx          3.8e-04    1.50e-03  4.9e-04 (0.32; golden n=1025)
rgb         1.0e-04    4.88e-04  3.8e-05 (0.08; golden n=1025)
sigma       1.9e-06    4.88e-04  6.5e-07 (0.00; golden n=1)
T1W         4.5e-06    1.95e-03  8.0e-06 (0.00; random n=1025)
T1b         1.6e-06    1.95e-03  2.8e-06 (0.00; random n=1025)
T2W         1.2e-06    1.95e-03  1.5e-06 (0.00; golden n=1025 explicit blend)
T2b         6.0e-07    1.95e-03  8.4e-07 (0.00; golden n=1025 explicit blend)
D1          5.5e-07    1.95e-03  4.0e-06 (0.00; random n=127)      D1[hash] 6.4e-06, D1[tm] 4.0e-06
D2          6.5e-06    1.95e-03  5.3e-06 (0.00; random n=127)
D3          2.0e-05    1.95e-03  1.3e-05 (0.01; golden n=129 explicit blend)
scale       2.2e-05    8.71e-05  2.2e-05 (0.25; golden n=127)
S1          1.3e-07    1.95e-03  1.8e-07 (0.00; golden n=1025)     S1[hash] 2.1e-07, S1[tcode] 1.8e-07
S2          6.4e-06    1.95e-03  6.4e-06 (0.00; golden n=257)
C1          1.2e-06    1.95e-03  1.1e-06 (0.00; golden n=1025)     C1[h16] 1.1e-06, C1[dir] 1.4e-07
C2          1.7e-05    1.95e-03  1.9e-07 (0.00; golden n=1025)
C3          3.7e-05    1.95e-03  1.7e-06 (0.00; random n=127)
d_feat[0]   5.9e-08    1.00e-06  5.8e-08 (0.06; random n=1)
d_feat[1]   5.0e-08    1.00e-06  5.0e-08 (0.05; random n=32)
d_feat[2]   4.4e-08    1.00e-06  4.4e-08 (0.04; random n=257)
d_feat[3]   3.5e-08    1.00e-06  4.3e-08 (0.04; random n=1)
Where no 16-bit rounding lands on its other neighbour the kernels and the restatement agree to fp32 round-off (every row of every
d_feat: 4e-8 .. 1.1e-6 of the row); the forward figures above that are single rows (golden: 12 of 1,025 rows of dx, 5 of rgb).
Plain float64 chain, n = 1,025: dx 1.3e-3 / 3.3e-4 of its maximum (golden / random; 2e-3), rgb 7.2e-4 / 4.1e-4 (3e-3), sigma 8.4e-3 /
1.6e-5 (2.5e-2).  Pads: 3,200 entries, exactly zero on both paths.  Anchor times: bits, nine cases.  g_scale under "deterministic"
against the default: 0 at n = 129 and 1,025 (2e-5).

Two findings of the first runs, neither a wrong kernel nor a wrong restatement; both changed what the test feeds, not a bound:
  * the backward entry is handed the REFERENCE's rgb and sigma (Chains.canon).  With the forward's own, one row in about a thousand
    had one of its three output derivatives d_rgb r (1 - r) on the other bf16 neighbour (the forward's sigmoid uses the fast
    exponential): that row's d_feat[3] moved by 2.9e-4 (random, row 8) and 4.8e-3 (golden, row 801) of the row, the tensor by 2.6e-5,
    where float32 sums alone leave 3.5e-8.
  * the rows are screened from the restatement alone (part4_reference.code_rows_ok, mask_rows_ok).  Before that

    49 of 54 passed: the canonical chain, random set, n >= 127 had every gradient behind C2 at 0.5-1 % (S1[hash] 1.2e-2, d_feat[3] 1.1e-2
    at n = 127).  One row, 124: its time code sat on a 16-bit tie (the same six rows differed in dx, rgb and sigma of BOTH parameter
    sets: the hardware sine against float64's), an operand took the other neighbour and one ReLU input of that row changed sign.
    The matched answer is not defined by the rounding points on such a row.

Mutations, run once on the GPU with the kernels unchanged and the reference mutated (not committed as tests):
  swap_blend_weights     22 of 54 fail: all 18 deformation sweep cases (d_feat[0], d_feat[2]) and the four explicit-blend cases
  drop_gate_derivative   22 of 54 fail: the same 22 (T1W, T1b, T2W, T2b)
  shift_time_band        38 of 54 fail: both chains' sweeps from n = 31 on, the explicit-blend cases and both plain-float64 cases;
                         n = 1 passes (row 0 is t = 0, where both bands give sin 0)
"""
import numpy as np
import pytest
import torch

import part4_reference as R
from conftest import golden

pytestmark = pytest.mark.gpu

WHICH = ("golden", "random")
P = lambda t: None if t is None else t.data_ptr()


class Chains:
    """the inputs of one parameter set on the GPU, the C entries on the first n rows, and the references (computed once per case)"""

    def __init__(self, which, g14):
        import project_nerf_amd  # noqa: F401
        from project_nerf_amd import ops, part4
        self.ops, self.part4, self.lib = ops, part4, ops._lib.load()
        self.c = c = R.chain_inputs(which, g14)
        self.dev = {k: c[k].cuda() for k in ("pts", "pts_c", "dirs", "t", "d_dx", "d_rgb", "d_sigma", "blend", "flat")}
        self.tables = [t.cuda() for t in c["tables"]]
        self.levels = [ops.HashLevelTable(*R.LEVELS_D)] * 3 + [ops.HashLevelTable(*R.LEVELS_C)]
        self.packed = part4.pack(self.dev["flat"])
        # the fp32 features the images hold as fp16
        self.feats = [ops.hash_encode_fwd(self.dev["pts_c" if k == 3 else "pts"], self.tables[k], self.levels[k], R.BOUND)[0].cpu() for k in range(4)]
        self.bounds = R.bounds(g14)
        self.yard = R.yardsticks(g14)
        self._ref = {}

    def reference(self, n, blend=False, rounded=True):
        key = (n, blend, rounded)
        if key not in self._ref:
            self._ref[key] = R.evaluate_inputs(self.c, self.feats, n, blend, rounded=rounded)
        return self._ref[key]

    def workspace(self, n, fill=None):
        ws = self.part4.Workspace(n, "cuda")
        if fill is not None:
            ws.buf.fill_(fill)
        return ws

    def image(self, ws, k, n, table=None, pts=None):
        """feature image k of the first n rows (or of other points / another table) into the workspace's slot"""
        pts = self.dev["pts_c" if k == 3 else "pts"][:n] if pts is None else pts
        self.ops.hash_encode_fwd_nat(pts.contiguous(), self.tables[k] if table is None else table, self.levels[k], R.BOUND, ws.nat(k), fp16=True)

    def deform(self, n, blend=None, t=None, ws=None, backward=True, flat=None, packed=None):
        """dict(dx, x_c, grads, d_feat[0..2]) of nerf_p4_deform_fwd (train) [+ nerf_p4_deform_bwd] on the first n rows; ws: a
        workspace whose three images the caller has written"""
        ops, lib, d = self.ops, self.lib, self.dev
        flat = d["flat"] if flat is None else flat
        packed = self.packed if packed is None else packed
        if ws is None:
            ws = self.workspace(n, 0xFF)
            for k in range(3):
                self.image(ws, k, n)
        t = d["t"][:n].contiguous() if t is None else t
        dx, xc = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n, 3), float("nan"), device="cuda")
        ops._lib.check(lib.nerf_p4_deform_fwd(P(packed), P(flat), P(ws.buf), P(d["pts"][:n].contiguous()), P(t), P(blend), n, P(dx), P(xc), 1,
                                              ops._stream()), "nerf_p4_deform_fwd")
        out = dict(dx=dx, x_c=xc)
        if backward:
            grads = torch.zeros(R.N_PARAMS, device="cuda")
            ops._lib.check(lib.nerf_p4_deform_bwd(P(packed), P(flat), P(ws.buf), P(d["d_dx"][:n].contiguous()), n, P(grads), None, None,
                                                  ops._stream()), "nerf_p4_deform_bwd")
            out.update(grads=grads, d_feat=[ws.d_feat(k).clone() for k in range(3)] + [None])
        return out

    def canon(self, n, backward=True, head=None):
        """dict(rgb, sigma, grads, d_feat[3]) of nerf_p4_canon_fwd (train) [+ nerf_p4_canon_bwd].  head = (rgb, sigma): the values the
        backward entry is HANDED (it takes them as inputs and forms the head's derivatives r (1 - r), 1 - exp(-sigma) from them)
        instead of the forward's own: with the reference's, both sides differentiate the head at the same numbers, and the fast
        exponential of the forward's sigmoid does not decide a bf16 rounding of the three output derivatives"""
        ops, lib, d = self.ops, self.lib, self.dev
        ws = self.workspace(n, 0xFF)
        self.image(ws, 3, n)
        rgb, sigma = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        t, dirs = d["t"][:n].contiguous(), d["dirs"][:n].contiguous()
        ops._lib.check(lib.nerf_p4_canon_fwd(P(self.packed), P(ws.buf), P(t), P(dirs), n, P(rgb), P(sigma), 1, ops._stream()), "nerf_p4_canon_fwd")
        out = dict(rgb=rgb, sigma=sigma)
        if backward:
            grads = torch.zeros(R.N_PARAMS, device="cuda")
            r_in, s_in = (rgb, sigma) if head is None else (head[0].float().cuda().contiguous(), head[1].float().cuda().contiguous())
            ops._lib.check(lib.nerf_p4_canon_bwd(P(self.packed), P(ws.buf), P(r_in), P(s_in), P(d["d_rgb"][:n].contiguous()),
                                                 P(d["d_sigma"][:n].contiguous()), n, P(grads), None, None, ops._stream()), "nerf_p4_canon_bwd")
            out.update(grads=grads, d_feat=[None] * 3 + [ws.d_feat(3).clone()])
        return out


@pytest.fixture(scope="module")
def bank():
    assert torch.cuda.is_available(), "gpu-marked test on a box without a HIP device"
    store, g14 = {}, golden("g14_part4")

    def get(which):
        if which not in store:
            store[which] = Chains(which, g14)
        return store[which]
    yield get
    store.clear()
    torch.cuda.empty_cache()


def hold(tag, ch, got, ref, chain):
    """every figure of ``got`` against the reference, printed next to its bound before the first assert; the gradient pads exactly zero"""
    bad = []
    for name, (fig, kind) in R.figures(got, ref, chains=(chain,)).items():
        lim = ch.bounds[name]
        print(f"FIG {tag} {name}: {fig:.3e} (bound {lim:.3e}, {fig / lim:.2f} of it; yardstick {ch.yard[name][0]:.2e})")
        if not fig <= lim:
            bad.append((name, fig, lim))
    for k, v in got.items():
        for t in (v if isinstance(v, list) else [v]):
            assert t is None or bool(torch.isfinite(t).all()), (tag, k, "not finite")
    assert float(got["grads"].cpu()[R.pad_mask()].abs().max()) == 0.0, (tag, "a pad row or column of the gradient vector was written")
    other = R.CANON_BLOCKS if chain == "deform" else R.DEFORM_BLOCKS
    assert all(float(R.live(got["grads"], name).abs().max()) == 0.0 for name in other), (tag, "the other chain's blocks were written")
    assert not bad, (tag, bad)


@pytest.mark.parametrize("n", R.SWEEP)
@pytest.mark.parametrize("which", WHICH)
def test_deformation_chain_against_the_matched_float64_chain(bank, which, n):
    ch = bank(which)
    got = ch.deform(n)
    ref = ch.reference(n)
    assert float((got["x_c"] - (ch.dev["pts"][:n] + got["dx"])).abs().max()) <= 2.0 ** -21       # x_c = x + dx: one fp32 rounding, contracted or not (|x_c| < 4)
    hold(f"deform {which} n={n}", ch, got, ref, "deform")


@pytest.mark.parametrize("n", R.SWEEP)
@pytest.mark.parametrize("which", WHICH)
def test_canonical_chain_against_the_matched_float64_chain(bank, which, n):
    ch = bank(which)
    ref = ch.reference(n)
    hold(f"canon {which} n={n}", ch, ch.canon(n, head=(ref["rgb"], ref["sigma"])), ref, "canon")


@pytest.mark.parametrize("n", [129, 1025])
@pytest.mark.parametrize("which", WHICH)
def test_explicit_blend_gives_every_grid_its_own_weight(bank, which, n):
    """random, non-normalised, pairwise distinct weights: each d_feat[k] carries w_k (what the mutation swap_blend_weights breaks)"""
    ch = bank(which)
    got = ch.deform(n, blend=ch.dev["blend"][:n].contiguous())
    hold(f"deform {which} n={n} explicit blend", ch, got, ch.reference(n, blend=True), "deform")
    w = ch.dev["blend"][:n]
    assert bool(((w[:, 0] != w[:, 1]) & (w[:, 1] != w[:, 2]) & (w[:, 0] != w[:, 2])).all())
    # one d(df) behind the three: d_feat[k] / w_k agree to the two fp32 roundings of the product and the quotient
    base = got["d_feat"][1].double() / w[:, 1:2].double()
    for k in (0, 2):
        assert R.rel_l2(got["d_feat"][k].double() / w[:, k:k + 1].double(), base) <= 4 * 2.0 ** -24, k


@pytest.mark.parametrize("which", WHICH)
def test_forward_against_the_plain_float64_chain(bank, which):
    """rounded=False, forward only, at the figures of test_fused_forward_vs_reference_golden (fp16 operands against fp32: dx 2e-3 of
    its maximum, rgb 3e-3, sigma 2.5e-2 of max(sigma, 1)): a reference bent towards the kernel would miss these"""
    ch, n = bank(which), 1025
    ref = ch.reference(n, rounded=False)
    dx = ch.deform(n, backward=False)["dx"].double().cpu()
    out = ch.canon(n, backward=False)
    e_d = float((dx - ref["dx"]).abs().max() / ref["dx"].abs().max())
    e_c = float((out["rgb"].double().cpu() - ref["rgb"]).abs().max())
    e_s = float(((out["sigma"].double().cpu() - ref["sigma"]).abs() / ref["sigma"].abs().clamp_min(1.0)).max())
    print(f"FIG plain float64 {which} n={n}: dx rel-to-max {e_d:.3e} (2e-3), |d rgb| {e_c:.3e} (3e-3), rel d sigma {e_s:.3e} (2.5e-2)")
    assert e_d < 2e-3 and e_c < 3e-3 and e_s < 2.5e-2


def test_gradient_pads_equal_what_the_fp32_module_path_leaves():
    """pad rows and columns of the network gradients (D1 columns 88.., D3 / C3 rows 3.., S1 columns 53.., C1 columns 43..; S2 has
    none): bit for bit what autograd through the fp32 module path leaves there, on the golden's own batch through part4.field"""
    from project_nerf_amd import part4
    from test_gpu_part4_engine import build_model
    T = torch.from_numpy
    pad = R.pad_mask()
    flats = []
    for fused in (True, False):
        m, g = build_model(fused)
        m.train()
        m.zero_grad()
        rgb, sigma, delta = m(T(g["pts"]).cuda(), T(g["dirs"]).cuda(), t=T(g["times"]).cuda())
        ((rgb * T(g["w_rgb"]).cuda()).sum() + sigma.sum() + (delta * T(g["w_dx"]).cuda()).sum()).backward()
        sd = dict(m.named_parameters())
        flats.append(torch.cat([sd[key].grad.reshape(-1) for key, _, _ in part4.MODULE_SLICES]).cpu())
    assert flats[0].numel() == R.N_PARAMS and float(flats[0][~pad].abs().max()) > 0.0
    print(f"FIG pads: {int(pad.sum())} entries, fp32 module path max |.| {float(flats[1][pad].abs().max()):.1e}, fused {float(flats[0][pad].abs().max()):.1e}")
    assert torch.equal(flats[0][pad], flats[1][pad])


@pytest.mark.parametrize("fill", ["other", "+0", "-0"])
@pytest.mark.parametrize("anchor", [0, 1, 2])
def test_anchor_times_take_the_anchor_grid_alone(bank, anchor, fill):
    """at t exactly 0, 0.5, 1 triangle_weights gives the one-hot row (the normaliser 1e-8f + 1 is 1.0f), so blend=None gives the bits
    of blend = that row, whatever the other two feature images hold: other finite features, zeros of either sign (the property
    deform_lattice_kernel relies on)"""
    ch, n = bank("random"), 129
    t = torch.full((n,), (0.0, 0.5, 1.0)[anchor], device="cuda")
    onehot = torch.zeros(n, 3, device="cuda")
    onehot[:, anchor] = 1.0
    want = ch.deform(n, blend=onehot, t=t)
    ws = ch.workspace(n, 0x00)
    for k in range(3):
        if k == anchor:
            ch.image(ws, k, n)
        elif fill == "other":
            ch.image(ws, k, n, table=ch.tables[(k + 1) % 3] * 1.7, pts=ch.dev["pts_c"][:n])
        elif fill == "-0":
            size = (n + 127) // 128 * 128 * 32
            ws.nat(k)[:2 * size].view(torch.int16).fill_(-32768)                 # fp16 -0 in every element of the image
    got = ch.deform(n, blend=None, t=t, ws=ws)
    assert torch.equal(got["dx"], want["dx"]) and torch.equal(got["x_c"], want["x_c"])
    assert torch.equal(got["d_feat"][anchor], want["d_feat"][anchor]) and float(want["d_feat"][anchor].abs().max()) > 0.0
    for k in range(3):
        if k != anchor:
            assert float(got["d_feat"][k].abs().max()) == 0.0 and float(want["d_feat"][k].abs().max()) == 0.0
    print(f"FIG anchor t={(0.0, 0.5, 1.0)[anchor]} other images {fill}: dx, x_c, d_feat equal bit for bit")


@pytest.mark.parametrize("n", [129, 1025])
def test_displacement_scale_gradient_under_deterministic(bank, n):
    """g_scale under option "deterministic" (one ordered add per workgroup) against its default-mode value, at the 2e-5 of
    tests/test_gpu_wgrad_sums.py"""
    ch = bank("golden")
    ops = ch.ops
    default = ch.deform(n)["grads"][R.SCALE].double()
    previous = ops.deterministic()
    ops.set_deterministic(True)
    try:
        det = [ch.deform(n)["grads"][R.SCALE].double() for _ in range(2)]
    finally:
        ops.set_deterministic(previous)
    fig = float((det[0] - default).abs() / default.abs())
    print(f"FIG g_scale deterministic vs default n={n}: {fig:.3e} (bound 2.0e-05)")
    assert torch.equal(det[0], det[1]) and fig <= 2e-5
