"""CPU-side checks of tests/part4_reference.py, the matched restatement of the two Part 4 chains (csrc/p4mlp.hip) that
tests/test_gpu_part4_chains.py holds the kernels to.  No GPU, no kernel:

(a) the restatement is the reference's Part 4: ``rounded=False`` composed with oracle.nerf_oracle.hash_encode, float64 autograd through
    x_canonical as well, reproduces golden g14b_part4_trained (the reference's NeuralField('part4') forward and autograd) at the
    bounds the fp32 module path is held to against the same golden (tests/test_gpu_part4_engine.py::G14B_FP32: delta 2e-6 of its
    maximum, rgb 2e-6, sigma 1e-5, gradients 2e-4).  None of them had to be widened (figures: Observed).
(b) the yardstick: the ``rounded=True`` chain with float32 sums (in four defined orders, part4_reference._mm) against itself with
    float64 sums, on the GPU tests' inputs (part4_reference.chain_inputs), per quantity.  The reference against itself in another summation order
    (tests/test_gpu_wgrad_sums.py::Part2.vs_matched's idea).  The GPU bound of a quantity is max(floor, 4 x yardstick), floors 2^-9
    (bf16-rounded), 2^-11 (fp16-rounded forward outputs), 1e-6 (fp32 sums only); the factor 4 covers the MFMA's k-block order and the
    fast exponential of the gate.  Asserted here: 4 x yardstick stays under the caps -- 2e-3 for forward quantities
    (test_deformation_chain_against_restatements' figure for the same operand format), 2e-2 for gradients
    (test_decoder_backward_vs_oracle_autograd's for the bf16 backward) -- for every case of the GPU sweep.
(c) every entry of part4_reference.MUTATIONS moves at least one quantity by more than 10 x its bound on those inputs.

Observed (this file, CPU)
-------------------------
(a) delta 1.05e-6 of max (2e-6), rgb 4.4e-7 (2e-6), sigma 4.7e-6 (1e-5); gradients: the four tables 1.4e-4 .. 1.6e-4, time modulation
    3.4e-5 .. 1.3e-4, displacement_scale 8.5e-5, deform_net 3.9e-5, sigma_net 1.9e-7, color_net 6.7e-7 (2e-4) -- the oracle's hash
    grid forms its trilinear weights in fp32, as the golden's did.  All inside G14B_FP32, none widened.
(b) per quantity, largest over the 22 cases and the four float32 orders: dx 3.8e-4, rgb 1.0e-4, sigma 1.9e-6; parameter blocks 1.3e-7
    (S1) .. 3.7e-5 (C3); input blocks 1.2e-7 .. 2.0e-6 (D1[hash]); scale 2.2e-5; the four d_feat 3.5e-8 .. 5.9e-8.  Largest
    4 x yardstick: 1.5e-3 (dx; cap 2e-3) and 1.5e-4 (C3; cap 2e-2).  The table and the GPU's figures: tests/test_gpu_part4_chains.py.
    Inputs that missed the dx cap and were changed: zero-mean D3 rows (one fp16 unit of one activation was 5.2e-4 .. 5.6e-4 of max |dx|).
(c) swap_blend_weights: d_feat[0] and d_feat[2] alone, by 8e5 .. 3e6 times their bound; drop_gate_derivative: T1W, T1b, T2W, T2b by
    1,700 .. 2,200 times; shift_time_band: 17 to 25 quantities, dx by 34 .. 199 times, S1[tcode] by ~180 .. 220 times.
"""
import numpy as np
import pytest
import torch

import part4_reference as R
from conftest import golden
from oracle import nerf_oracle as O

T = torch.from_numpy
G14B_FP32 = dict(delta=2e-6, rgb=2e-6, sigma=1e-5, grads=2e-4)          # tests/test_gpu_part4_engine.py (a gpu-marked module)


@pytest.fixture(scope="module")
def g14():
    return golden("g14_part4")


def inputs(g14, which):
    R.yardstick_case(which, 1, False, g14)
    return R._YARD[("inputs", which)]


def test_plain_float64_chain_reproduces_the_reference_golden():
    g = golden("g14b_part4_trained")
    flat = R.golden_flat(g).double().requires_grad_(True)
    tables = [T(g["t:" + k]).double().view(-1, 2).requires_grad_(True)
              for k in ("deform_grid_start", "deform_grid_mid", "deform_grid_end", "canonical_repr")]
    lv_d, lv_c = O.hash_grid_levels(*R.LEVELS_D), O.hash_grid_levels(*R.LEVELS_C)
    pts, dirs, t = T(g["pts"]), T(g["dirs"]), T(g["times"]).reshape(-1)
    x01 = O.hash_normalise(pts.double(), R.BOUND)
    feats = [O.hash_encode(lv_d, tables[k], x01) for k in range(3)]
    dx, xc = R.deform_chain(flat, feats, t, pts.double(), rounded=False)
    rgb, sigma = R.canon_chain(flat, O.hash_encode(lv_c, tables[3], O.hash_normalise(xc, R.BOUND)), t, dirs, rounded=False)
    ((rgb * T(g["w_rgb"]).double()).sum() + sigma.sum() + (dx * T(g["w_dx"]).double()).sum()).backward()
    e_d = float(np.abs(dx.detach().numpy() - g["delta"]).max() / np.abs(g["delta"]).max())
    e_c = float(np.abs(rgb.detach().numpy() - g["rgb"]).max())
    e_s = float((np.abs(sigma.detach().numpy()[:, None] - g["sigma"]) / np.maximum(np.abs(g["sigma"]), 1.0)).max())
    print(f"FIG (a) g14b forward: delta_x rel-to-max {e_d:.3e} ({G14B_FP32['delta']:.0e}), |d rgb| {e_c:.3e} ({G14B_FP32['rgb']:.0e}), "
          f"rel d sigma {e_s:.3e} ({G14B_FP32['sigma']:.0e})")
    gf = flat.grad
    mine = {"time_modulation.net.0.weight": gf[R.T1W:R.T1B], "time_modulation.net.0.bias": gf[R.T1B:R.T2W],
            "time_modulation.net.2.weight": gf[R.T2W:R.T2B], "time_modulation.net.2.bias": gf[R.T2B:R.D1],
            "deform_decoder.deform_net.params": gf[R.D1:R.S1], "decoder.sigma_net.params": gf[R.S1:R.C1],
            "decoder.color_net.params": gf[R.C1:R.SCALE], "deform_decoder.displacement_scale": gf[R.SCALE:],
            "deform_grid_start.encoding.params": tables[0].grad, "deform_grid_mid.encoding.params": tables[1].grad,
            "deform_grid_end.encoding.params": tables[2].grad, "canonical_repr.encoding.params": tables[3].grad}
    bad, checked = [], 0
    for k, v in g.items():
        if not k.startswith("g:"):
            continue
        fig = R.rel_l2(mine[k[2:]].reshape(-1), T(v).reshape(-1))
        print(f"FIG (a) g14b gradient {k[2:]}: rel-L2 {fig:.3e} (bound {G14B_FP32['grads']:.0e})")
        checked += 1
        if not fig < G14B_FP32["grads"]:
            bad.append((k, fig))
    assert checked == 12 and not bad, bad
    assert e_d < G14B_FP32["delta"] and e_c < G14B_FP32["rgb"] and e_s < G14B_FP32["sigma"], (e_d, e_c, e_s)


def test_rounded_chain_differs_from_the_plain_chain_by_its_rounding_alone(g14):
    """rounded=True differs from rounded=False by the rounding alone: forward within the fp16 / bf16 formats' reach, and the pads of
    the gradient vector exactly zero in both"""
    c, feats = inputs(g14, "random")
    a = R.evaluate_inputs(c, feats, 129, rounded=True)
    b = R.evaluate_inputs(c, feats, 129, rounded=False)
    f = R.figures(a, b)
    print("FIG rounded vs plain float64: " + " ".join(f"{k}={v[0]:.2e}" for k, v in f.items()))
    assert f["dx"][0] < 2e-3 and f["rgb"][0] < 3e-3 and f["sigma"][0] < 2.5e-2
    assert all(0.0 < v[0] < 0.05 for v in f.values()), f
    pad = R.pad_mask()
    assert int(pad.sum()) == 64 * 8 + 13 * 64 + 64 * 11 + 64 * 5 + 13 * 64
    assert float(a["grads"][pad].abs().max()) == 0.0 and float(b["grads"][pad].abs().max()) == 0.0


@pytest.mark.parametrize("which,n,blend", R.YARD_CASES)
def test_yardstick_stays_under_the_caps(g14, which, n, blend):
    yard, _ = R.yardstick_case(which, n, blend, g14)
    bad = []
    for name, (fig, kind) in yard.items():
        cap = R.CAP_FORWARD if kind == "fwd" else R.CAP_GRAD
        print(f"FIG (b) {which} n={n} blend={'explicit' if blend else 'None'} {name}: yardstick {fig:.3e}, 4 x = {4 * fig:.3e} (cap {cap:.0e})")
        if not 4 * fig <= cap:
            bad.append((name, fig, cap))
    assert not bad, bad


def test_pooled_yardsticks_and_the_bounds_they_give(g14):
    """the table the GPU tests use: per quantity the largest yardstick over the cases, and max(floor, 4 x it)"""
    yard, bounds = R.yardsticks(g14), R.bounds(g14)
    assert len(yard) == 3 + 13 + 6 + 4
    tightest = min(b for k, b in bounds.items() if yard[k][1] == "grad")
    for name, (fig, kind) in yard.items():
        cap = R.CAP_FORWARD if kind == "fwd" else R.CAP_GRAD
        print(f"FIG (b) pooled {name} [{kind}]: yardstick {fig:.3e}, GPU bound {bounds[name]:.3e} (cap {cap:.0e})")
        assert 0.0 <= fig and bounds[name] <= cap, (name, fig, bounds[name], cap)
    assert tightest <= 0.12 / 5                                   # against the 0.12-0.15 Part 4's network gradients were held to
    assert all(b <= 0.12 / 5 for k, b in bounds.items() if yard[k][1] != "fwd"), bounds


@pytest.mark.parametrize("blend", [False, True])
@pytest.mark.parametrize("which", ["golden", "random"])
@pytest.mark.parametrize("mutate", [m for m in R.MUTATIONS if m is not None])
def test_each_mutation_is_seen_at_ten_times_a_bound(g14, mutate, which, blend):
    n = 1025
    _, ref = R.yardstick_case(which, n, blend, g14)
    bounds = R.bounds(g14)
    c, feats = inputs(g14, which)
    wrong = R.evaluate_inputs(c, feats, n, blend, rounded=True, mutate=mutate)
    moved = R.figures(wrong, ref)
    seen = {k: v[0] / bounds[k] for k, v in moved.items() if v[0] > 10 * bounds[k]}
    print(f"FIG (c) {mutate} {which} blend={'explicit' if blend else 'None'}: moved by more than 10 x their bound: " +
          ", ".join(f"{k} {v:.0f}x" for k, v in seen.items()))
    assert seen, (mutate, moved)
    if mutate == "swap_blend_weights":
        assert "d_feat[0]" in seen and "d_feat[2]" in seen and set(seen) <= {"d_feat[0]", "d_feat[2]"}, seen      # backward only, grids 0 and 2 only
