"""The tail of every training step against float64 references, through the C ABI, on one MI355X (pytest -m gpu):
csrc/composite.hip (nerf_composite_mse_bwd, nerf_composite_mse_reg_bwd) against oracle.composite_mse_reg and
csrc/adam.hip (squared norm + TV sign codes, clip + AdamW, the small group, nerf_adam_step, nerf_f32_to_f16) against
oracle.tv_clip_adamw.  The two references are pinned by tests/test_step_tail_oracle.py.  One process, one GPU.

S = 1 is left out of the compositing sweep: oracle.composite builds the far interval with full_like(step[:, :1]),
which is empty there.

Tolerances -- compositing.  The project's numbers for this operation against fp32 references (test_gpu_parity):
pixel rtol 1e-6 / atol 1e-7, loss rtol 1e-5, d_rgb rtol 1e-5 (atol 1e-10), d_sigma 2e-5 of the ray's largest reference
|d_sigma|, amax rtol 1e-4.  m = sum w extra takes the pixel's, d_extra takes d_rgb's, reg takes the loss's.  The absolute
floor under d_rgb / d_extra comes from the rounding of alpha = 1 - exp(-sigma delta) (see check_composite).  Every case
first measures the YARDSTICK: oracle.composite_mse_reg in fp32 against itself in float64 on the case's own inputs, in
the same metric.  bound = max(project's number, 4 x yardstick): the kernel reduces in a tree where the oracle runs a
sequential cumprod, so it is owed a small multiple of what plain fp32 reaches, not equality.  Nothing is derived
from the kernel's output.  Metrics are written |x - ref| / (|ref| + atol / rtol) so that one figure compares with rtol.

Tolerances -- optimiser.  One step from identical fp32 state is a handful of fp32 operations.  Yardstick: the same
step by oracle.tv_clip_adamw in fp32 on the CPU against float64, per quantity; bound = max(4 x yardstick, 8 x 2^-23)
(the kernel folds 1/bc1 and 1/sqrt(bc2) into fp32 constants and the compiler may contract to FMA; 8 x 2^-23: eight
roundings of one ulp, the floor below which a yardstick over a handful of elements is luck), params never above the
project's rtol 2e-5 / atol 2e-7 in the project's metric |d| / (|ref| + 1e-2) ("p_project").  Metrics under the yardstick rule:
params |d| / (|ref| + |p before| + 1e-2) (a difference of two rounded numbers: see step_figures); exp_avg, exp_avg_sq and the
rewritten gradient |d| / (|ref| + rms(ref)).  normsq: the project's 1e-5 relative.  The AdamW pass is checked from ITS inputs: the
reference takes the squared norm the kernel's workspace actually holds (checked on its own to 1e-5).  Codes, the fp16
copy, untouched buffers and guard elements: bit for bit.

Finding kept in the tests: the C ABI carries beta1 / beta2 as floats and the library forms 1 - beta^step from them, so against
torch's double 0.999 params differ by up to 1.5e-5 (project's metric) at steps 1 and 2 -- under the project's 2e-5, far above the
yardstick.  The reference is given the betas the kernel gets (HYP below).

Figures of the run this file was written on (one MI355X, 261 tests in 4 s); every test prints its own (pytest -s).

Observed
--------
Maxima over the cases of each row, as yardstick (fp32 oracle vs float64) / largest bound applied / seen on the GPU.

compositing      d_sigma (of ray max)        d_rgb                       d_extra                     pixel                       loss
S=   2           5.2e-07/2.0e-05/4.0e-07     3.3e-07/1.0e-05/3.3e-07     3.6e-07/1.0e-05/3.6e-07     2.2e-08/1.0e-06/2.2e-08     1.7e-08/1.0e-05/1.2e-07
S=   3           6.0e-06/2.4e-05/2.2e-06     3.4e-07/1.0e-05/3.4e-07     6.4e-08/1.0e-05/6.4e-08     9.3e-08/1.0e-06/9.3e-08     5.1e-08/1.0e-05/7.5e-08
S=  64           1.9e-06/2.0e-05/8.9e-07     1.1e-06/1.0e-05/7.3e-07     3.1e-07/1.0e-05/2.8e-07     2.8e-07/1.1e-06/1.5e-07     8.3e-08/1.0e-05/1.7e-07
S=  65           7.6e-07/2.0e-05/1.2e-06     8.7e-07/1.0e-05/5.7e-07     6.1e-07/1.0e-05/3.5e-07     3.3e-07/1.3e-06/3.3e-07     1.4e-07/1.0e-05/2.0e-07
S= 129           6.7e-07/2.0e-05/6.1e-07     6.8e-07/1.0e-05/4.5e-07     2.9e-07/1.0e-05/2.9e-07     2.2e-07/1.0e-06/0.0e+00     1.5e-07/1.0e-05/1.7e-07
S= 192           7.0e-07/2.0e-05/9.2e-07     5.8e-07/1.0e-05/4.0e-07     2.3e-07/1.0e-05/2.7e-07     2.1e-07/1.0e-06/0.0e+00     5.3e-08/1.0e-05/9.6e-08
S= 256           4.8e-07/2.0e-05/6.7e-07     2.3e-07/1.0e-05/2.7e-07     4.7e-07/1.0e-05/7.4e-07     1.5e-07/1.0e-06/0.0e+00     2.0e-08/1.0e-05/2.5e-07
S= 320           1.2e-06/2.0e-05/2.3e-06     3.9e-07/1.0e-05/7.2e-07     8.6e-07/1.0e-05/9.1e-07     2.0e-07/1.0e-06/2.9e-07     2.2e-07/1.0e-05/4.2e-07
S= 448           1.0e-06/2.0e-05/1.5e-06     6.6e-07/1.0e-05/7.8e-07     2.8e-07/1.0e-05/2.6e-07     2.2e-07/1.0e-06/2.6e-07     5.4e-08/1.0e-05/1.0e-07
S= 576           2.9e-07/2.0e-05/1.2e-06     3.9e-07/1.0e-05/3.9e-07     7.2e-07/1.0e-05/9.6e-07     1.3e-07/1.0e-06/3.0e-07     1.9e-07/1.0e-05/1.0e-06
S= 832           8.2e-07/2.0e-05/8.0e-07     9.0e-07/1.0e-05/1.1e-06     3.4e-07/1.0e-05/3.7e-07     3.5e-07/1.4e-06/6.5e-07     2.9e-07/1.0e-05/5.6e-08
S=1024           1.4e-06/2.0e-05/1.7e-06     3.9e-07/1.0e-05/8.8e-07     2.0e-07/1.0e-05/6.0e-07     2.7e-07/1.1e-06/0.0e+00     2.2e-07/1.0e-05/2.4e-07
many rays        7.0e-06/2.8e-05/9.0e-06     1.2e-06/1.0e-05/1.1e-06     2.9e-08/1.0e-05/2.8e-08     4.7e-07/1.9e-06/5.6e-07     1.3e-07/1.0e-05/6.5e-07
reg alone        1.9e-03/7.8e-03/1.9e-03     0.0e+00/1.0e-05/0.0e+00     4.8e-07/1.0e-05/6.7e-07     2.1e-07/1.0e-06/2.1e-07     0.0e+00/1.0e-05/0.0e+00
engine ratio     1.8e-06/2.0e-05/1.4e-06     3.9e-07/1.0e-05/7.6e-07     2.2e-09/1.0e-05/2.2e-09     1.8e-07/1.0e-06/0.0e+00     1.4e-07/1.0e-05/9.3e-08
zero far         rest 1.0e-06/2.0e-05/1.8e-06, far sample 7.1e-06/2.8e-05/7.0e-06 (its own relative error; saturated rays set the yardstick)
all cases: m 5.1e-07/2.0e-06/3.9e-07, reg 1.8e-06/1.0e-05/1.5e-06, amax 7.6e-07/1.0e-04/1.1e-06

optimiser        params (operands metric)    params (project's metric)   exp_avg                     exp_avg_sq                  rewritten g
accumulate       1.7e-07/9.5e-07/1.1e-07     4.2e-07/2.0e-05/7.3e-07     6.6e-08/9.5e-07/3.7e-08     7.9e-08/9.5e-07/4.2e-08     -
adam             9.0e-08/9.5e-07/8.8e-08     1.9e-07/2.0e-05/2.5e-07     7.9e-08/9.5e-07/4.5e-08     8.3e-08/9.5e-07/8.3e-08     -
adamw_clip_step  1.6e-07/9.5e-07/9.2e-08     4.4e-07/2.0e-05/3.0e-07     6.8e-08/9.5e-07/4.5e-08     7.3e-08/9.5e-07/4.6e-08     -
codes+adamw_tv   2.7e-07/1.1e-06/2.2e-07     3.6e-06/2.0e-05/2.8e-06     8.4e-08/9.5e-07/6.8e-08     9.2e-08/9.5e-07/4.9e-08     -
pieces=2         1.7e-07/9.5e-07/9.4e-08     6.8e-07/2.0e-05/5.1e-07     7.6e-08/9.5e-07/4.2e-08     7.7e-08/9.5e-07/4.3e-08     -
pieces=3         1.7e-07/9.5e-07/9.4e-08     6.8e-07/2.0e-05/5.1e-07     7.6e-08/9.5e-07/4.2e-08     7.7e-08/9.5e-07/4.3e-08     -
pieces=7         1.7e-07/9.5e-07/9.4e-08     6.8e-07/2.0e-05/5.1e-07     7.6e-08/9.5e-07/4.2e-08     7.7e-08/9.5e-07/4.3e-08     -
rewriting        2.1e-07/9.5e-07/2.0e-07     1.7e-06/2.0e-05/1.6e-06     7.6e-08/9.5e-07/7.3e-08     7.7e-08/9.5e-07/7.7e-08     4.2e-08/9.5e-07/4.2e-08
small            2.7e-07/1.1e-06/2.4e-07     1.5e-06/2.0e-05/1.0e-06     7.6e-08/9.5e-07/7.6e-08     8.5e-08/9.5e-07/8.5e-08     -
splits           1.1e-07/9.5e-07/7.9e-08     3.9e-07/2.0e-05/3.3e-07     6.9e-08/9.5e-07/4.2e-08     8.9e-08/9.5e-07/4.1e-08     -
"""
import math

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

F64 = torch.float64
EINVAL = -22
SENTINEL = 12345.0
EPS8 = 8.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a box without a HIP device")
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import _lib
    _lib.load()
    return _lib


def P(t):
    return None if t is None else t.data_ptr()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def report(name, figures):
    print(f"[step-tail] {name}: " + ", ".join(f"{k} yard {y:.2e} bound {b:.2e} seen {s:.2e}" for k, (y, b, s) in figures.items()))


# ============================================================================================== compositing + loss backward
def composite_case(R, S, seed, slot_map, bg_kind, zero_far=False):
    """fp32 inputs on the CPU.  Densities are relu'd (exact zeros) except on the far sample, which is > 0 unless zero_far"""
    gen = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(R, S, generator=gen) * 4 + 2, dim=-1).values
    d = torch.randn(R, 3, generator=gen)
    d = d / d.norm(dim=-1, keepdim=True) * (0.5 + torch.rand(R, 1, generator=gen))
    sig = torch.relu(torch.randn(R, S, generator=gen)) * 3
    if not zero_far:
        sig[:, -1] = torch.rand(R, generator=gen) * 2 + 0.05
    rgb = torch.rand(R, S, 3, generator=gen)
    ext = torch.randn(R, S, 3, generator=gen) * 0.1
    target = torch.rand(R, 3, generator=gen)
    bg = {"none": None, "one": torch.rand(1, 3, generator=gen), "ray": torch.rand(R, 3, generator=gen)}[bg_kind]
    case = dict(R=R, S=S, z=z, d=d, target=target, bg=bg, slots=None)
    if not slot_map:
        case.update(rgb=rgb.reshape(-1, 3), sig=sig.reshape(-1), ext=ext.reshape(-1, 3), ray_of_row=torch.arange(R).repeat_interleave(S),
                    far_row=torch.arange(R) * S + S - 1)
        return case
    active = torch.rand(R, S, generator=gen) < 0.3
    if R >= 3:
        active[0] = False                      # one ray with nothing active
        active[1] = True                       # one fully active
    n, spare = int(active.sum()), 5            # five rows of the compact arrays that no sample maps to
    perm = torch.randperm(n + spare, generator=gen)[:n]
    slots = torch.full((R, S), -1, dtype=torch.int32)
    slots[active] = perm.to(torch.int32)
    c_rgb, c_sig, c_ext = torch.rand(n + spare, 3, generator=gen), torch.rand(n + spare, generator=gen), torch.randn(n + spare, 3, generator=gen)
    c_rgb[perm], c_sig[perm], c_ext[perm] = rgb[active], sig[active], ext[active]
    ray_of_row = torch.full((n + spare,), -1, dtype=torch.long)
    ray_of_row[perm] = torch.arange(R)[:, None].expand(R, S)[active]
    far_row = torch.where(active[:, -1], slots[:, -1].long(), torch.full((R,), -1, dtype=torch.long))
    case.update(rgb=c_rgb, sig=c_sig, ext=c_ext, slots=slots, ray_of_row=ray_of_row, far_row=far_row)
    return case


def rel(x, ref, floor):
    x, ref = x.double(), ref.double()
    return float(((x - ref).abs() / (ref.abs() + floor)).max()) if ref.numel() else 0.0


def ray_scaled(ds, ref, ray_of_row, R, rows):
    """max over ``rows`` of |ds - ref| / (largest |ref| over the same ray's rows among ``rows``); the rays that take part"""
    top = torch.zeros(R, dtype=F64)
    top.scatter_reduce_(0, ray_of_row[rows], ref[rows].abs(), reduce="amax")
    err = (ds[rows].double() - ref[rows]).abs() / (top[ray_of_row[rows]] + 1e-300)
    return (float(err.max()) if err.numel() else 0.0), top


def composite_metrics(got, ref, case, split_far):
    """one figure per quantity, each to be compared with its rtol"""
    mapped = ref["mapped"]
    rows = torch.nonzero(mapped).reshape(-1)
    out = {"pixel": rel(got["pixel"], ref["pixel"], 0.1), "d_rgb": rel(got["d_rgb"][mapped], ref["d_rgb"][mapped], ref["floor_rgb"]),
           "loss": abs(got["loss"] - ref["loss"]) / (abs(ref["loss"]) + 1e-300)}
    if ref["d_extra"] is not None:
        out["m"] = rel(got["m"], ref["m"], 0.1)
        out["d_extra"] = rel(got["d_extra"][mapped], ref["d_extra"][mapped], ref["floor_extra"])
        out["reg"] = abs(got["reg"] - ref["reg"]) / (abs(ref["reg"]) + 1e-300)
    else:
        out["amax"] = abs(got["amax"] - ref["amax"]) / (abs(ref["amax"]) + 1e-300)
    if not split_far:
        out["d_sigma"], _ = ray_scaled(got["d_sigma"], ref["d_sigma"], case["ray_of_row"], case["R"], rows)
    else:
        # (b): the far sample by its own relative error, the rest scaled by the ray's maximum over the rest
        far = case["far_row"][case["far_row"] >= 0]
        is_far = torch.zeros_like(mapped)
        is_far[far] = True
        out["d_sigma_rest"], _ = ray_scaled(got["d_sigma"], ref["d_sigma"], case["ray_of_row"], case["R"], torch.nonzero(mapped & ~is_far).reshape(-1))
        out["d_sigma_far"] = rel(got["d_sigma"][far], ref["d_sigma"][far], 1e-30)
    return out


PROJECT = {"pixel": 1e-6, "m": 1e-6, "d_rgb": 1e-5, "d_extra": 1e-5, "loss": 1e-5, "reg": 1e-5, "amax": 1e-4, "d_sigma": 2e-5,
           "d_sigma_rest": 2e-5, "d_sigma_far": 2e-5}


def run_composite(lib, case, entry, use_ws, outs, loss_weight, reg_weight, ref):
    """two launches into preloaded accumulators; returns what the kernel left, the accumulators reduced to one call's share"""
    L = lib.load()
    R, S = case["R"], case["S"]
    dev = lambda t, dt=None: None if t is None else (t if dt is None else t.to(dt)).contiguous().cuda()
    rgb, sig, ext, z, d, target, bg, slots = (dev(case[k]) for k in ("rgb", "sig", "ext", "z", "d", "target", "bg", "slots"))
    n = rgb.shape[0]
    d_rgb, d_sig, d_ext = (torch.full(s, SENTINEL, device="cuda") for s in ((n, 3), (n,), (n, 3)))
    pred = torch.full((R, 3), SENTINEL, device="cuda") if outs else None
    emap = torch.full((R, 3), SENTINEL, device="cuda") if (outs and entry == "reg") else None
    ws = torch.zeros(lib.SUM_WS_FLOATS, device="cuda") if use_ws else None
    pre_loss, pre_reg = np.float32(0.5 * ref["loss"]), np.float32(0.5 * ref["reg"])
    acc = torch.tensor([pre_loss, pre_reg, 0.25 * ref["amax"], 4.0 * ref["amax"]], dtype=torch.float32).cuda()
    high = float(acc[3])
    bg_rows = 0 if bg is None else bg.shape[0]
    for call in range(2):
        if entry == "mse":
            rc = L.nerf_composite_mse_bwd(P(rgb), P(sig), P(slots), P(z), P(d), P(bg), bg_rows, P(target), loss_weight, R, S, P(pred),
                                          P(acc[0:1]), P(d_rgb), P(d_sig), P(acc[2 + call:3 + call]), P(ws), None)
        else:
            rc = L.nerf_composite_mse_reg_bwd(P(rgb), P(sig), P(slots), P(z), P(d), P(bg), bg_rows, P(target), loss_weight, P(ext), reg_weight,
                                              R, S, P(pred), P(emap), P(acc[0:1]), P(acc[1:2]), P(d_rgb), P(d_sig), P(d_ext), P(ws), None)
        lib.check(rc, "composite")
    torch.cuda.synchronize()
    a = acc.cpu().double()
    got = {"d_rgb": d_rgb.cpu(), "d_sigma": d_sig.cpu(), "d_extra": d_ext.cpu(), "pixel": ref["pixel"] if pred is None else pred.cpu(),
           "m": ref["m"] if emap is None else emap.cpu(), "loss": (float(a[0]) - float(pre_loss)) / 2.0, "reg": (float(a[1]) - float(pre_reg)) / 2.0,
           "amax": float(a[2])}
    if entry == "mse":
        assert float(a[3]) == high, "a running maximum above the result must stay as it is"
        assert float(a[1]) == float(pre_reg), "nerf_composite_mse_bwd has no regulariser output"
    else:
        assert float(a[2]) == float(np.float32(0.25 * ref["amax"])), "nerf_composite_mse_reg_bwd has no maximum output"
    # rows that no sample maps to keep the sentinel, every mapped row lost it
    mapped = ref["mapped"]
    for name, t in (("d_rgb", got["d_rgb"]), ("d_sigma", got["d_sigma"])) + ((("d_extra", got["d_extra"]),) if entry == "reg" else ()):
        flat = t.reshape(t.shape[0], -1)
        assert bool((flat[~mapped] == SENTINEL).all()), f"{name}: a row of a skipped sample was written"
        assert not bool((flat[mapped] == SENTINEL).any()), f"{name}: a mapped row was not written"
    if entry == "mse":
        assert bool((got["d_extra"] == SENTINEL).all())
    return got


def check_composite(lib, name, case, entry, use_ws, outs, loss_weight, reg_weight, split_far=False, need_rays=True):
    kw = dict(extra=case["ext"] if entry == "reg" else None, reg_weight=reg_weight if entry == "reg" else 0.0, slots=case["slots"])
    ref = O.composite_mse_reg(case["rgb"], case["sig"], case["z"], case["d"], case["bg"], case["target"], loss_weight, **kw)
    f32 = O.composite_mse_reg(case["rgb"], case["sig"], case["z"], case["d"], case["bg"], case["target"], loss_weight, dtype=torch.float32, **kw)
    # absolute floor of d_rgb = w g and d_extra = w g_m (the issue gives their rtol only): w = alpha T with alpha = 1 - e, whose fp32
    # value carries an absolute error of up to 2^-24 from the subtraction plus ~2 ulp of e <= 2^-23 from expf, so |dw| <= 3 x 2^-24 and
    # |d d_rgb| <= 3 x 2^-24 max|g|; times the 4 the kernel is owed; never below the project's atol 1e-10 (floor = atol / rtol)
    g_pix = 2.0 * loss_weight * float((ref["pixel"] - case["target"].double()).abs().max())
    g_m = 2.0 * kw["reg_weight"] * float(ref["m"].abs().max())
    ref["floor_rgb"] = max(1e-10, 12.0 * 2.0 ** -24 * g_pix) / 1e-5
    ref["floor_extra"] = max(1e-10, 12.0 * 2.0 ** -24 * g_m) / 1e-5
    if not split_far:
        # condition of metric (a): every ray takes part -- no far sample of order 1e9 hides the others of its ray
        rows = torch.nonzero(ref["mapped"]).reshape(-1)
        _, top = ray_scaled(ref["d_sigma"], ref["d_sigma"], case["ray_of_row"], case["R"], rows)
        assert float(top.max()) < 1e3, "a ray's largest reference |d_sigma| is not < 1e3: the case does not test what it says"
    yard = composite_metrics(f32, ref, case, split_far)
    got = run_composite(lib, case, entry, use_ws, outs, loss_weight, reg_weight, ref)
    seen = composite_metrics(got, ref, case, split_far)
    figures = {k: (yard[k], max(PROJECT[k], 4.0 * yard[k]), seen[k]) for k in seen}
    report(name, figures)
    bad = {k: v for k, v in figures.items() if not v[2] <= v[1]}
    assert not bad, f"{name}: (yardstick, bound, seen) {bad}"
    return figures


S_SWEEP = [2, 3, 64, 65, 129, 192, 256, 320, 448, 576, 832, 1024]          # K = 1 1 1 2 3 3 4 6 8 12 16 16 samples per lane


def sweep_cases():
    out = []
    for i, S in enumerate(S_SWEEP):
        for e, entry in enumerate(("mse", "reg")):
            j = 2 * i + e
            out.append((entry, S, (1, 3, 41)[j % 3], (j // 3) % 2 == 0, ("none", "one", "ray")[(j // 2) % 3], (j // 5) % 2 == 0, (j // 7) % 2 == 0))
    for entry in ("mse", "reg"):                                    # the full product of the options at one ragged S
        for slot_map in (False, True):
            for bg in ("none", "one", "ray"):
                for use_ws in (True, False):
                    out.append((entry, 65, 41, slot_map, bg, use_ws, not use_ws if bg == "one" else use_ws))
    return out


@pytest.mark.parametrize("entry,S,R,slot_map,bg,use_ws,outs", sweep_cases())
def test_composite_mse_bwd_sweep_vs_float64(lib, entry, S, R, slot_map, bg, use_ws, outs):
    case = composite_case(R, S, 1000 * S + R, slot_map, bg)
    check_composite(lib, f"composite {entry} S={S} R={R} slots={int(slot_map)} bg={bg} ws={int(use_ws)} outs={int(outs)}", case, entry, use_ws,
                    outs, 1.0 / (3 * R), 0.05 / (3 * R))


@pytest.mark.parametrize("entry", ["mse", "reg"])
@pytest.mark.parametrize("use_ws", [True, False])
@pytest.mark.parametrize("slot_map", [False, True])
def test_composite_mse_bwd_more_rays_than_waves(lib, entry, use_ws, slot_map):
    """R above four times the launch's workgroup cap (CUs x 8 with sum_ws, CUs x composite_wgs_per_cu without): every wave
    takes several rays and sums several losses"""
    per_cu = 8 if use_ws else max(1, lib.get_option("composite_wgs_per_cu"))
    R = 4 * cus() * per_cu * 2 + 7
    case = composite_case(R, 65, 77, slot_map, "one")
    check_composite(lib, f"composite {entry} many rays R={R} ws={int(use_ws)} slots={int(slot_map)}", case, entry, use_ws, True, 1.0 / (3 * R),
                    0.05 / (3 * R))


@pytest.mark.parametrize("entry,S", [("mse", 64), ("reg", 129), ("mse", 17), ("reg", 1024)])
def test_composite_mse_bwd_exact_zero_densities_far_sample_on_its_own(lib, entry, S):
    """metric (b): exact zeros everywhere, the far sample included (its derivative is of order 1e9 there)"""
    case = composite_case(41, S, 5 + S, False, "ray", zero_far=True)
    assert int((case["sig"].view(41, S)[:, -1] == 0).sum()) >= 10
    check_composite(lib, f"composite {entry} zero-far S={S}", case, entry, True, True, 1.0 / (3 * 41), 0.05 / (3 * 41), split_far=True)


@pytest.mark.parametrize("S,slot_map,use_ws", [(64, True, True), (192, False, False), (3, False, True)])
def test_composite_regulariser_alone(lib, S, slot_map, use_ws):
    """loss_weight = 0: d_sigma and d_extra are the regulariser's alone, d_rgb is zero, the target does not matter"""
    case = composite_case(41, S, 31 + S, slot_map, "one")
    case["target"] = case["target"] * 100.0 - 7.0
    fig = check_composite(lib, f"composite reg alone S={S}", case, "reg", use_ws, True, 0.0, 0.7)
    assert fig["d_sigma"][2] <= fig["d_sigma"][1] and fig["loss"][2] == 0.0


@pytest.mark.parametrize("S,R", [(64, 41), (256, 64)])
def test_composite_regulariser_at_the_engines_ratio(lib, S, R):
    case = composite_case(R, S, 91 + S, True, "one")
    check_composite(lib, f"composite engines' ratio S={S}", case, "reg", True, False, 1.0 / (3 * R), 1e-4 / (3 * R))
    # and the regulariser's share of d_sigma is visible at that ratio: the same call without it differs from the reference
    ref = O.composite_mse_reg(case["rgb"], case["sig"], case["z"], case["d"], case["bg"], case["target"], 1.0 / (3 * R), case["ext"],
                              1e-4 / (3 * R), case["slots"])
    off = O.composite_mse_reg(case["rgb"], case["sig"], case["z"], case["d"], case["bg"], case["target"], 1.0 / (3 * R), case["ext"], 0.0,
                              case["slots"])
    print(f"[step-tail] engines' ratio: regulariser's share of d_sigma {float((ref['d_sigma'] - off['d_sigma']).abs().max()):.2e} of "
          f"{float(ref['d_sigma'].abs().max()):.2e}")


# ============================================================================================================ optimiser
G = 16          # guard elements on both sides of every buffer (64 bytes of floats: the 16-byte alignment of the view stays)
# the C ABI carries the betas as floats and the library forms 1 - beta^step from what it got: the reference gets the same values
# (against the double 0.999 the bias correction differs by 1.3e-5 at step 1 and 2, up to 1.5e-5 of params in the metric below)
HYP = dict(beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=1e-8)


def staircase(n, gen):
    """runs of equal values of lengths 1..9: ties on every position of a 4-chunk and across chunk, round and seam borders"""
    runs = torch.arange(n) % 9 + 1
    vals = torch.randn(n, generator=gen)
    return torch.repeat_interleave(vals, runs)[:n].contiguous()


def table_values(kind, n, gen):
    if kind == "random":
        return torch.randn(n, generator=gen) * 0.1
    if kind == "const":
        return torch.full((n,), 0.37)
    if kind == "zero":
        return torch.zeros(n)
    if kind == "stairs":
        return staircase(n, gen)
    if kind == "monotone":
        return torch.cumsum(torch.rand(n, generator=gen) + 1e-3, 0) * 1e-3
    raise ValueError(kind)


class Guarded:
    """a device buffer with guard elements around the view the kernel gets; ``mis``: the view starts that many elements late"""

    def __init__(self, data, mis=0, fill=SENTINEL):
        n = data.numel()
        self.full = torch.full((n + 2 * G + mis,), fill, dtype=data.dtype).cuda() if data.dtype != torch.uint8 else \
            torch.full((n + 2 * G + mis,), 0xAA, dtype=torch.uint8).cuda()
        self.fill = 0xAA if data.dtype == torch.uint8 else fill
        self.lo, self.n = G + mis, n
        self.view = self.full[self.lo:self.lo + n]
        self.view.copy_(data)

    def cpu(self):
        return self.view.cpu()

    def guards_intact(self):
        f = self.full.cpu()
        return bool((f[:self.lo] == self.fill).all()) and bool((f[self.lo + self.n:] == self.fill).all())


def opt_state(n, seed, kind="random", mis=0, g_scale=1e-2):
    gen = torch.Generator().manual_seed(seed)
    p = table_values(kind, n, gen)
    g = torch.randn(n, generator=gen) * g_scale
    m = torch.randn(n, generator=gen) * g_scale                      # non-zero moments: every output depends on the gradient's scale
    v = (torch.randn(n, generator=gen) * g_scale) ** 2 + 1e-3 * g_scale ** 2
    return {k: Guarded(t, mis) for k, t in (("p", p), ("g", g), ("m", m), ("v", v))}


def rms_rel(x, ref):
    x, ref = x.double(), ref.double()
    return float(((x - ref).abs() / (ref.abs() + float(ref.pow(2).mean().sqrt()) + 1e-300)).max())


def step_figures(before, after, ref_kw, name, shadow=None, grad_after=None):
    """``before`` / ``after``: the kernel's actual p, g, m, v (CPU fp32) around ONE step; the float64 reference and the fp32
    yardstick start from ``before``"""
    ref = O.tv_clip_adamw(before["p"], before["g"], before["m"], before["v"], **ref_kw)
    f32 = O.tv_clip_adamw(before["p"], before["g"], before["m"], before["v"], dtype=torch.float32, **ref_kw)
    # params = p (1 - lr wd) - update is a difference of two fp32 numbers, each rounded at its own size: where they cancel the error is
    # a few ulp of the OPERANDS, so the yardstick metric scales by |ref| + |p before| + 1e-2; the project's metric (|ref| + 1e-2) and its
    # rtol 2e-5 stay as the ceiling beside it
    p0 = before["p"].double().abs()
    operands = lambda a, b: float(((a.double() - b).abs() / (b.abs() + p0 + 1e-2)).max())
    figures = {"p_project": (rel(f32["p"], ref["p"], 1e-2), 2e-5, rel(after["p"], ref["p"], 1e-2))}
    for k, metric in (("p", operands), ("m", rms_rel), ("v", rms_rel)):
        yard = metric(f32[k], ref[k])
        figures[k] = (yard, max(4.0 * yard, EPS8), metric(after[k], ref[k]))
    if grad_after is not None:
        figures["g"] = (rms_rel(f32["grad"], ref["grad"]), max(4.0 * rms_rel(f32["grad"], ref["grad"]), EPS8), rms_rel(grad_after, ref["grad"]))
    report(name, figures)
    bad = {k: v for k, v in figures.items() if not v[2] <= v[1]}
    assert not bad, f"{name}: (yardstick, bound, seen) {bad}"
    if shadow is not None:
        assert torch.equal(shadow.view(torch.int16), after["p"].half().view(torch.int16)), f"{name}: fp16 copy != params.half()"
    return ref


def snapshot(st):
    return {k: st[k].cpu() for k in ("p", "g", "m", "v")}


def codes_equal(got, want, n):
    """bit for bit, the padding codes past n masked"""
    got, want = got.clone(), want.clone()
    if n % 4:
        mask = (1 << (2 * (n % 4))) - 1
        got[-1] &= mask
        want[-1] &= mask
    return torch.equal(got, want)


def codes_step(lib, name, n, n_tables, tv_w, kind="random", mis=0, grad_scale=1.0, max_norm=0.0, wd=0.0, step=2, seed=0, lr=1e-2,
               lr_split=0, lr_hi=0.0, clipping=None, g_scale=1e-2):
    """nerf_tv_normsq_codes + nerf_adamw_clip_step_tv over n_tables equal tables, each pass checked from its own inputs"""
    L = lib.load()
    st = opt_state(n, seed, kind, mis, g_scale)
    shadow = Guarded(torch.zeros(n, dtype=torch.float16), 0 if mis == 0 else 4 * ((mis + 3) // 4), fill=77.0)
    nb = (n + 3) // 4
    codes = Guarded(torch.full((nb,), 0xAA, dtype=torch.uint8))
    ws = torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda")
    ws[0] = 3.0e7                                                     # a storing call overwrites whatever the norm held
    seg = n // n_tables
    tables = [(k * seg, seg, tv_w) for k in range(n_tables)]
    before = snapshot(st)
    lib.check(L.nerf_tv_normsq_codes(P(st["p"].view), P(st["g"].view), n, n_tables, tv_w, grad_scale, P(ws), 0,
                                     P(codes.view) if tv_w != 0.0 else None, None), name)
    torch.cuda.synchronize()
    kw = dict(step=step, lr=lr, weight_decay=wd, tables=tables, grad_scale=grad_scale, max_norm=max_norm, lr_split=lr_split, lr_hi=lr_hi, **HYP)
    ref0 = O.tv_clip_adamw(before["p"], before["g"], before["m"], before["v"], **kw)
    normsq = float(ws[0])
    assert abs(normsq - ref0["normsq"]) <= 1e-5 * ref0["normsq"], (name, normsq, ref0["normsq"])
    if tv_w != 0.0 and seg > 1:
        assert codes_equal(codes.cpu(), ref0["codes"], n), f"{name}: TV sign codes"
    mid = snapshot(st)
    assert all(torch.equal(mid[k], before[k]) for k in mid), f"{name}: the codes pass changed a buffer it only reads"
    if clipping is not None:
        norm = math.sqrt(ref0["normsq"])
        assert abs(norm - max_norm) > 0.01 * max_norm and (norm > max_norm) == clipping, (name, norm, max_norm)
    lib.check(L.nerf_adamw_clip_step_tv(P(st["p"].view), P(st["g"].view), P(st["m"].view), P(st["v"].view), n, step, lr, 0.9, 0.999, 1e-8, wd,
                                        P(ws), max_norm, grad_scale, P(codes.view) if tv_w != 0.0 else None, n, tv_w, seg, 0.0, 0, lr_split, lr_hi,
                                        P(shadow.view), None), name)
    torch.cuda.synchronize()
    after = snapshot(st)
    assert torch.equal(after["g"], before["g"]), f"{name}: the gradient buffer was written"
    step_figures(before, after, dict(kw, normsq_total=normsq), name, shadow.cpu())
    assert all(b.guards_intact() for b in (*st.values(), shadow, codes)), f"{name}: a guard element was written"
    return st, ws


SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4099, 10007, 4 * 1237]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mis", [0, 1, 2])
def test_codes_and_adamw_tv_sizes_and_alignments(lib, n, mis):
    """one table, TV on; mis = 0 and n % 4 = 0: the fast kernel, otherwise the generic one"""
    codes_step(lib, f"codes n={n} mis={mis}", n, 1, 0.3, mis=mis, grad_scale=0.5, max_norm=1e-3, wd=1e-2, step=2, seed=n + mis,
               kind="stairs" if n % 2 else "random")


@pytest.mark.parametrize("n_tables", [1, 2, 3, 4])
@pytest.mark.parametrize("tv_w", [0.0, 0.7])
@pytest.mark.parametrize("mis", [0, 1])
def test_codes_and_adamw_tv_tables_and_seams(lib, n_tables, tv_w, mis):
    """seg % 4 == 0; stairs put ties on both sides of every seam"""
    for seg, kind in ((4, "stairs"), (1236, "stairs"), (2048, "random")):
        codes_step(lib, f"codes tables={n_tables} seg={seg} tv={tv_w} mis={mis}", seg * n_tables, n_tables, tv_w, kind=kind, mis=mis,
                   grad_scale=0.25, max_norm=0.0, wd=0.0, step=1, seed=seg + n_tables)


@pytest.mark.parametrize("kind", ["const", "zero", "stairs", "monotone", "random"])
@pytest.mark.parametrize("n,n_tables", [(4 * 1237, 1), (3 * 1024, 3), (10007, 1)])
def test_codes_and_adamw_tv_ties(lib, kind, n, n_tables):
    codes_step(lib, f"codes ties {kind} n={n}", n, n_tables, 1.3, kind=kind, grad_scale=2.0, max_norm=0.0, wd=1e-5, step=1000, seed=n)


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("clip", ["off", "clipping", "not clipping"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_codes_and_adamw_tv_steps_clip_and_decay(lib, step, clip, wd):
    # |g * 3| ~ 3e-2 * sqrt(4096) ~ 1.9: max_norm 0.3 clips, 30 does not
    max_norm = {"off": 0.0, "clipping": 0.3, "not clipping": 30.0}[clip]
    codes_step(lib, f"codes step={step} clip={clip} wd={wd}", 4096, 2, 0.05, grad_scale=3.0, max_norm=max_norm, wd=wd, step=step, seed=step,
               clipping=None if clip == "off" else clip == "clipping")


def test_clip_keeps_the_1e_6_of_clip_grad_norm(lib):
    """a tiny norm and a tinier max_norm: coef = max_norm / (norm + 1e-6) is far from max_norm / norm"""
    codes_step(lib, "codes tiny norm", 1024, 1, 0.0, grad_scale=1.0, max_norm=1e-7, wd=0.0, step=2, seed=5, clipping=True, g_scale=2e-8)
    codes_step(lib, "codes tiny norm (generic)", 1023, 1, 0.0, grad_scale=1.0, max_norm=1e-7, wd=0.0, step=2, seed=6, clipping=True, g_scale=2e-8)


def test_codes_fast_kernel_several_rounds_and_the_clamped_last_chunk(lib):
    """tv_blocks = 1: 1024 threads x 4 chunks per round; n / 4 = 2 * 4096 + 1024 + 37 takes three rounds, the last one partial in
    its second chunk (the loads past the end are clamped to the last chunk and masked)"""
    previous = lib.get_option("tv_blocks")
    try:
        for blocks, n4 in ((1, 2 * 4096 + 1024 + 37), (3, 3 * 3 * 4096 + 5)):
            lib.set_option("tv_blocks", blocks)
            codes_step(lib, f"codes fast rounds tv_blocks={blocks}", 4 * n4, 1, 0.9, kind="stairs", grad_scale=0.5, max_norm=0.1, step=3, seed=n4)
            codes_step(lib, f"codes fast rounds tv_blocks={blocks} 4 tables", 16 * (n4 // 4), 4, 0.9, kind="stairs", grad_scale=0.5, step=3, seed=n4)
    finally:
        lib.set_option("tv_blocks", previous)


def test_accumulate_two_groups_under_one_norm(lib):
    """group A stores its squared norm, group B adds: both step under the clip of the sum"""
    L = lib.load()
    a, b = opt_state(4096, 1), opt_state(1025, 2, mis=1)
    ca, ws = Guarded(torch.zeros(1024, dtype=torch.uint8)), torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda")
    ws[0] = 99.0
    lib.check(L.nerf_tv_normsq_codes(P(a["p"].view), P(a["g"].view), 4096, 2, 0.4, 0.5, P(ws), 0, P(ca.view), None), "A")
    lib.check(L.nerf_tv_normsq_codes(P(b["p"].view), P(b["g"].view), 1025, 1, 0.0, 0.5, P(ws), 1, None, None), "B")
    torch.cuda.synchronize()
    ba, bb = snapshot(a), snapshot(b)
    kwa = dict(step=4, lr=1e-2, weight_decay=1e-2, tables=[(0, 2048, 0.4), (2048, 2048, 0.4)], grad_scale=0.5, max_norm=0.05, **HYP)
    kwb = dict(step=4, lr=3e-3, weight_decay=0.0, tables=[], grad_scale=0.5, max_norm=0.05, **HYP)
    ra, rb = O.tv_clip_adamw(ba["p"], ba["g"], ba["m"], ba["v"], **kwa), O.tv_clip_adamw(bb["p"], bb["g"], bb["m"], bb["v"], **kwb)
    total, normsq = ra["normsq"] + rb["normsq"], float(ws[0])
    assert abs(normsq - total) <= 1e-5 * total and math.sqrt(total) > 1.01 * 0.05
    lib.check(L.nerf_adamw_clip_step_tv(P(a["p"].view), P(a["g"].view), P(a["m"].view), P(a["v"].view), 4096, 4, 1e-2, 0.9, 0.999, 1e-8, 1e-2, P(ws),
                                        0.05, 0.5, P(ca.view), 4096, 0.4, 2048, 0.0, 0, 0, 0.0, None, None), "A")
    lib.check(L.nerf_adamw_clip_step_tv(P(b["p"].view), P(b["g"].view), P(b["m"].view), P(b["v"].view), 1025, 4, 3e-3, 0.9, 0.999, 1e-8, 0.0, P(ws),
                                        0.05, 0.5, None, 0, 0.0, 0, 0.0, 0, 0, 0.0, None, None), "B")
    torch.cuda.synchronize()
    step_figures(ba, snapshot(a), dict(kwa, normsq_total=normsq), "accumulate A")
    step_figures(bb, snapshot(b), dict(kwb, normsq_total=normsq), "accumulate B")
    assert all(x.guards_intact() for x in (*a.values(), *b.values(), ca))


@pytest.mark.parametrize("tv_split,lr_split", [(3 * 1024, 3 * 1024), (3 * 1024, 0), (0, 1024), (3 * 1024, 9999), (9999, 2048)])
def test_adamw_tv_splits(lib, tv_split, lr_split):
    """three tables of 1024 (weight 0.8) then one of 2052 (weight 0.05): Part 4's layout; tv_split / lr_split at 0, inside and >= n"""
    L = lib.load()
    n_lo, seg_lo, n_hi, n = 3 * 1024, 1024, 2052, 3 * 1024 + 2052
    st = opt_state(n, 11, "stairs")
    codes, shadow = Guarded(torch.zeros(n // 4, dtype=torch.uint8)), Guarded(torch.zeros(n, dtype=torch.float16), fill=77.0)
    ws = torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda")
    lib.check(L.nerf_tv_normsq_codes(P(st["p"].view), P(st["g"].view), n_lo, 3, 0.8, 0.5, P(ws), 0, P(codes.view), None), "lo")
    lib.check(L.nerf_tv_normsq_codes(P(st["p"].view[n_lo:]), P(st["g"].view[n_lo:]), n_hi, 1, 0.05, 0.5, P(ws), 1, P(codes.view[n_lo // 4:]), None), "hi")
    torch.cuda.synchronize()
    before = snapshot(st)
    layout = [(0, 1024, 0.8), (1024, 1024, 0.8), (2048, 1024, 0.8), (n_lo, n_hi, 0.05)]
    full = O.tv_clip_adamw(before["p"], before["g"], before["m"], before["v"], step=2, lr=1e-2, tables=layout, grad_scale=0.5, **HYP)
    normsq = float(ws[0])
    assert abs(normsq - full["normsq"]) <= 1e-5 * full["normsq"]
    assert codes_equal(codes.cpu(), full["codes"], n)
    # the step: tv_split says which (weight, table size) a chunk takes -- the codes are those of the real layout
    if tv_split == n_lo:
        tables = layout
    elif tv_split == 0:                                      # everything on the high side's scale
        tables = None
        scale_lo = scale_hi = 0.05 / (n_hi - 1)
    else:                                                    # everything on the low side's scale
        tables = None
        scale_lo = scale_hi = 0.8 / (seg_lo - 1)
    lib.check(L.nerf_adamw_clip_step_tv(P(st["p"].view), P(st["g"].view), P(st["m"].view), P(st["v"].view), n, 2, 1e-2, 0.9, 0.999, 1e-8, 1e-2,
                                        P(ws), 0.02, 0.5, P(codes.view), tv_split, 0.8, seg_lo, 0.05, n_hi, lr_split, 4e-3, P(shadow.view), None),
              "step")
    torch.cuda.synchronize()
    if tables is None:
        # one scale over the real layout's signs: weight = scale * (elems - 1) per table
        tables = [(o, e, scale_lo * (e - 1)) for o, e, _ in layout]
    kw = dict(step=2, lr=1e-2, weight_decay=1e-2, tables=tables, grad_scale=0.5, max_norm=0.02, lr_split=lr_split, lr_hi=4e-3, normsq_total=normsq, **HYP)
    step_figures(before, snapshot(st), kw, f"splits tv={tv_split} lr={lr_split}", shadow.cpu())
    assert all(x.guards_intact() for x in (*st.values(), codes, shadow))


def test_refused_arguments(lib):
    """entries that need alignment or multiples of 4 return NERF_EINVAL and do not run"""
    L = lib.load()
    st = opt_state(64, 1)
    ws, codes, h = torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(80, dtype=torch.float16, device="cuda")
    p, g, m, v = (st[k].view for k in ("p", "g", "m", "v"))
    before = snapshot(st)
    args = (P(m), P(v), 32, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, P(ws), 0.0, 1.0)
    assert L.nerf_tv_normsq_codes_piece(P(p[1:]), P(g[1:]), 32, 64, 0, 0.1, 1.0, P(ws), 0, P(codes[16:]), None) == EINVAL      # misaligned
    assert L.nerf_tv_normsq_codes_piece(P(p), P(g), 30, 64, 0, 0.1, 1.0, P(ws), 0, P(codes[16:]), None) == EINVAL             # n % 4
    assert L.nerf_tv_normsq_codes_piece(P(p), P(g), 32, 16, 0, 0.1, 1.0, P(ws), 0, P(codes[16:]), None) == EINVAL             # table < piece
    assert L.nerf_tv_normsq_codes(P(p), P(g), 30, 3, 0.1, 1.0, P(ws), 0, P(codes), None) == EINVAL                            # seg % 4
    assert L.nerf_tv_normsq_codes(P(p), P(g), 32, 5, 0.1, 1.0, P(ws), 0, P(codes), None) == EINVAL                            # five tables
    assert L.nerf_tv_normsq_accum_tables(P(p), P(g), 30, 3, 0.1, 1.0, P(ws), None) == EINVAL
    assert L.nerf_adamw_clip_step_tv(P(p), P(g), *args, P(codes), 6, 0.1, 6, 0.1, 26, 0, 0.0, None, None) == EINVAL            # tv_split % 4
    assert L.nerf_adamw_clip_step_tv(P(p), P(g), *args, P(codes), 8, 0.1, 8, 0.1, 24, 10, 1e-3, None, None) == EINVAL          # lr_split % 4
    assert L.nerf_adamw_clip_step_tv(P(p), P(g), *args, None, 0, 0.0, 0, 0.0, 0, 0, 0.0, P(h[1:]), None) == EINVAL             # fp16 copy unaligned
    assert L.nerf_adamw_clip_step_shadow(P(p), P(g), P(m), P(v), 32, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, P(ws), 0.0, 1.0, P(h[1:]), None) == EINVAL
    assert L.nerf_adamw_clip_step_shadow(P(p), P(g), P(m), P(v), 32, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, P(ws), 0.0, 1.0, None, None) == EINVAL
    assert L.nerf_clip_adamw_small(P(p), P(g), P(m), P(v), 65537, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0, None, 0, None) == EINVAL
    assert L.nerf_adam_step(P(p), P(g), P(m), P(v), 32, 0, 1e-2, 0.9, 0.999, 1e-8, 0.0, None, None) == EINVAL                  # step 0
    torch.cuda.synchronize()
    after = snapshot(st)
    assert all(torch.equal(after[k], before[k]) for k in after) and float(ws.abs().sum()) == 0.0 and int(codes.sum()) == 0


# ------------------------------------------------------------------------------------------------------------- pieces
def cuts_for(n, pieces, gen):
    if pieces == 2:
        return [0, 4, n]                                           # a 4-element piece
    inner = sorted(set((torch.randperm(n // 4 - 2, generator=gen)[:pieces - 1] + 1).mul(4).tolist()))
    return [0] + inner + [n]


@pytest.mark.parametrize("pieces", [2, 3, 7])
@pytest.mark.parametrize("kind", ["stairs", "random", "const"])
@pytest.mark.parametrize("max_norm", [0.0, 0.05])
@pytest.mark.parametrize("layout", ["shared", "own"])
def test_pieces_equal_the_whole_table(lib, pieces, kind, max_norm, layout):
    """ONE table cut at multiples of 4 (stairs / const: ties on the cuts), stepped piece by piece with the halo bits of sharded.py,
    against the whole-table reference and, without a clip, the whole-table kernel bit for bit.  layout "shared": all pieces in one
    code buffer (codes[-1] of a piece is the last byte of the piece before it, which must survive); "own": every piece in a buffer of
    its own behind 16 spare bytes, as sharded.py lays a rank's slice out (codes[-1] is the only place its s[-1] comes from)"""
    L = lib.load()
    n, tv_w, gs, step, lr, wd = 4 * 1237, 0.6, 0.5, 3, 1e-2, 1e-2
    gen = torch.Generator().manual_seed(pieces)
    cuts = cuts_for(n, pieces, gen)
    st, whole = opt_state(n, 21, kind), opt_state(n, 21, kind)
    before = snapshot(st)
    shadow, shadow_w = Guarded(torch.zeros(n, dtype=torch.float16), fill=77.0), Guarded(torch.zeros(n, dtype=torch.float16), fill=77.0)
    ws, ws_w = torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda"), torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda")
    ws[0] = 55.0
    spans = [(a, b - a, (1 if a > 0 else 0) | (2 if b < n else 0)) for a, b in zip(cuts[:-1], cuts[1:])]
    if layout == "shared":
        codes = Guarded(torch.zeros(n // 4, dtype=torch.uint8))      # codes[-1] of the first piece is a guard byte: never written (halo 0)
        code_of = [codes.view[a // 4:] for a, _, _ in spans]
        bufs = [codes]
    else:
        bufs = [Guarded(torch.zeros(16 + cnt // 4, dtype=torch.uint8)) for _, cnt, _ in spans]
        code_of = [b.view[16:] for b in bufs]
    for i, (a, cnt, halo) in enumerate(spans):
        lib.check(L.nerf_tv_normsq_codes_piece(P(st["p"].view[a:]), P(st["g"].view[a:]), cnt, n, halo, tv_w, gs, P(ws), 0 if i == 0 else 1,
                                               P(code_of[i]), None), "piece normsq")
    torch.cuda.synchronize()
    kw = dict(step=step, lr=lr, weight_decay=wd, tables=[(0, n, tv_w)], grad_scale=gs, max_norm=max_norm, **HYP)
    ref0 = O.tv_clip_adamw(before["p"], before["g"], before["m"], before["v"], **kw)
    normsq = float(ws[0])
    assert abs(normsq - ref0["normsq"]) <= 1e-5 * ref0["normsq"]
    if layout == "shared":
        # every piece's last byte holds its s[n-1] towards the next piece: the buffer equals the whole table's codes
        assert torch.equal(codes.cpu(), ref0["codes"]), "piece codes (halo bit 1 / codes[-1])"
    else:
        for (a, cnt, halo), b in zip(spans, bufs):
            own = b.cpu()
            assert torch.equal(own[16:], ref0["codes"][a // 4:(a + cnt) // 4]), "piece codes (halo bit 1)"
            assert bool((own[:15] == 0).all()) and int(own[15]) & 0x3F == 0, "bytes before the piece: only the top code of codes[-1] is written"
            assert int(own[15]) >> 6 == (int(ref0["codes"][a // 4 - 1]) >> 6 if halo & 1 else 0), "codes[-1]: the sign of p[0] - p[-1]"
    if max_norm > 0.0:
        assert math.sqrt(ref0["normsq"]) > 1.01 * max_norm
    for i, (a, cnt, halo) in enumerate(spans):
        lib.check(L.nerf_adamw_clip_step_tv_piece(P(st["p"].view[a:]), P(st["g"].view[a:]), P(st["m"].view[a:]), P(st["v"].view[a:]), cnt, step, lr,
                                                  0.9, 0.999, 1e-8, wd, P(ws), max_norm, gs, P(code_of[i]), tv_w, n, halo & 1,
                                                  P(shadow.view[a:]), None), "piece adamw")
    torch.cuda.synchronize()
    after = snapshot(st)
    step_figures(before, after, dict(kw, normsq_total=normsq), f"pieces={pieces} {kind} max_norm={max_norm} {layout}", shadow.cpu())
    assert torch.equal(after["g"], before["g"])
    assert all(x.guards_intact() for x in (*st.values(), *bufs, shadow))
    # the whole-table kernels on a copy
    cw = Guarded(torch.zeros(n // 4, dtype=torch.uint8))
    lib.check(L.nerf_tv_normsq_codes(P(whole["p"].view), P(whole["g"].view), n, 1, tv_w, gs, P(ws_w), 0, P(cw.view), None), "whole normsq")
    lib.check(L.nerf_adamw_clip_step_tv(P(whole["p"].view), P(whole["g"].view), P(whole["m"].view), P(whole["v"].view), n, step, lr, 0.9, 0.999, 1e-8,
                                        wd, P(ws_w), max_norm, gs, P(cw.view), n, tv_w, n, 0.0, 0, 0, 0.0, P(shadow_w.view), None), "whole adamw")
    torch.cuda.synchronize()
    assert torch.equal(cw.cpu(), ref0["codes"])
    assert abs(float(ws_w[0]) - normsq) <= 1e-5 * normsq
    if max_norm == 0.0:                                              # with a clip the two differ through normsq (another order of summation)
        aw = snapshot(whole)
        assert all(torch.equal(aw[k].view(torch.int32), after[k].view(torch.int32)) for k in aw), "pieces != whole table, bit for bit"
        assert torch.equal(shadow_w.cpu().view(torch.int16), shadow.cpu().view(torch.int16))


# -------------------------------------------------------------------------------------------------- the one-launch small group
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 4097, 65536])
@pytest.mark.parametrize("zero_grads", [0, 1])
@pytest.mark.parametrize("want_normsq", [False, True])
def test_clip_adamw_small(lib, n, zero_grads, want_normsq):
    """every workgroup sums the whole gradient itself: one clip for all (clipping case, compared elementwise)"""
    L = lib.load()
    st = opt_state(n, n + zero_grads, mis=n % 3)
    out = torch.full((3,), SENTINEL, device="cuda")
    before = snapshot(st)
    gs, step, lr, wd = 0.5, 2, 1e-2, 1e-2
    ref0 = O.tv_clip_adamw(before["p"], before["g"], before["m"], before["v"], step=step, lr=lr, grad_scale=gs, **HYP)
    max_norm = 0.25 * math.sqrt(ref0["normsq"])                       # clipping by a factor of four, whatever n
    lib.check(L.nerf_clip_adamw_small(P(st["p"].view), P(st["g"].view), P(st["m"].view), P(st["v"].view), n, step, lr, 0.9, 0.999, 1e-8, wd,
                                      max_norm, gs, P(out[1:2]) if want_normsq else None, zero_grads, None), "small")
    torch.cuda.synchronize()
    after = snapshot(st)
    o = out.cpu()
    assert float(o[0]) == SENTINEL and float(o[2]) == SENTINEL
    if want_normsq:
        assert abs(float(o[1]) - ref0["normsq"]) <= 1e-5 * ref0["normsq"]
    else:
        assert float(o[1]) == SENTINEL
    # the kernel's own norm is not visible without normsq_out: the reference clips by its own; 1e-5 on the norm is 5e-6 on the
    # coefficient, which the yardstick rule does not cover -- so the clip is taken from the kernel's norm where it is given and the
    # case without it is compared with the case with it bit for bit below
    kw = dict(step=step, lr=lr, weight_decay=wd, grad_scale=gs, max_norm=max_norm, **HYP)
    if want_normsq:
        step_figures(before, after, dict(kw, normsq_total=float(o[1])), f"small n={n} zero={zero_grads}")
    else:
        twin = opt_state(n, n + zero_grads, mis=n % 3)
        lib.check(L.nerf_clip_adamw_small(P(twin["p"].view), P(twin["g"].view), P(twin["m"].view), P(twin["v"].view), n, step, lr, 0.9, 0.999, 1e-8,
                                          wd, max_norm, gs, P(out[1:2]), zero_grads, None), "small twin")
        torch.cuda.synchronize()
        tw = snapshot(twin)
        assert all(torch.equal(tw[k].view(torch.int32), after[k].view(torch.int32)) for k in tw)
    if zero_grads:
        assert float(after["g"].abs().max()) == 0.0 and not bool(torch.signbit(after["g"]).any())
    else:
        assert torch.equal(after["g"], before["g"])
    assert all(x.guards_intact() for x in st.values())


# --------------------------------------------------------------------------------------------------------- rewriting forms
@pytest.mark.parametrize("n,n_tables,mis", [(10007, 1, 0), (10007, 1, 1), (4 * 1237, 1, 0), (3 * 1236, 3, 0), (4 * 1024, 4, 2), (5, 1, 0), (1, 1, 0)])
@pytest.mark.parametrize("kind", ["stairs", "random"])
def test_rewriting_tv_normsq_and_adamw_clip_step(lib, n, n_tables, mis, kind):
    """nerf_tv_normsq / _accum / _accum_tables leave g * grad_scale + TV in the gradient buffer; nerf_adamw_clip_step[_shadow] steps from it"""
    L = lib.load()
    st = opt_state(n, 3 * n + mis, kind, mis)
    shadow = Guarded(torch.zeros(n, dtype=torch.float16), 0 if mis == 0 else 4, fill=77.0)
    ws = torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda")
    before = snapshot(st)
    tv_w, gs, step, lr, wd, max_norm = 0.4, 0.5, 2, 1e-2, 1e-2, 0.02
    seg = n // n_tables
    if n_tables == 1:
        ws[0] = 31.0                                                   # nerf_tv_normsq zeroes first
        lib.check(L.nerf_tv_normsq(P(st["p"].view), P(st["g"].view), n, tv_w, gs, P(ws), None), "tv_normsq")
    else:
        lib.check(L.nerf_tv_normsq_accum_tables(P(st["p"].view), P(st["g"].view), n, n_tables, tv_w, gs, P(ws), None), "tv_normsq_accum_tables")
    torch.cuda.synchronize()
    kw = dict(step=step, lr=lr, weight_decay=wd, tables=[(k * seg, seg, tv_w) for k in range(n_tables)], grad_scale=gs, max_norm=max_norm, **HYP)
    ref0 = O.tv_clip_adamw(before["p"], before["g"], before["m"], before["v"], **kw)
    normsq = float(ws[0])
    assert abs(normsq - ref0["normsq"]) <= 1e-5 * ref0["normsq"]
    mid = snapshot(st)
    assert all(torch.equal(mid[k], before[k]) for k in ("p", "m", "v"))
    if n_tables == 1:                                                  # ... and _accum adds a second group's norm to it
        other = opt_state(1023, 9)
        lib.check(L.nerf_tv_normsq_accum(P(other["p"].view), P(other["g"].view), 1023, 0.0, 1.0, P(ws), None), "tv_normsq_accum")
        torch.cuda.synchronize()
        extra = float(other["g"].cpu().double().pow(2).sum())
        assert abs(float(ws[0]) - (ref0["normsq"] + extra)) <= 1e-5 * (ref0["normsq"] + extra)
        assert torch.equal(other["g"].cpu(), snapshot(other)["g"]) and other["g"].guards_intact()
        normsq = float(ws[0])
    fn = L.nerf_adamw_clip_step_shadow if n % 2 else L.nerf_adamw_clip_step
    tail = (P(shadow.view), None) if n % 2 else (None,)
    lib.check(fn(P(st["p"].view), P(st["g"].view), P(st["m"].view), P(st["v"].view), n, step, lr, 0.9, 0.999, 1e-8, wd, P(ws), max_norm, 1.0, *tail), "step")
    torch.cuda.synchronize()
    after = snapshot(st)
    assert torch.equal(after["g"], mid["g"])
    # the rewritten gradient against the reference's; then the step from the kernel's own rewritten gradient (grad_scale 1, no tables)
    step_figures(before, dict(after, p=after["p"]), dict(kw, normsq_total=normsq), f"rewriting n={n} tables={n_tables} mis={mis} {kind} (from g)",
                 grad_after=mid["g"])
    kw2 = dict(step=step, lr=lr, weight_decay=wd, grad_scale=1.0, max_norm=max_norm, normsq_total=normsq, **HYP)
    step_figures(mid, after, kw2, f"rewriting n={n} tables={n_tables} mis={mis} {kind} (from the rewritten g)", shadow.cpu() if n % 2 else None)
    assert all(x.guards_intact() for x in (*st.values(), shadow))


def test_adamw_clip_step_scales_the_norm_it_is_given(lib):
    """grad_scale of nerf_adamw_clip_step applies to the gradient AND to the norm it clips by (normsq is of the unscaled gradient)"""
    L = lib.load()
    n = 4099
    st, ws = opt_state(n, 8), torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda")
    lib.check(L.nerf_tv_normsq(P(st["p"].view), P(st["g"].view), n, 0.0, 1.0, P(ws), None), "normsq")
    torch.cuda.synchronize()
    before, raw = snapshot(st), float(ws[0])
    assert torch.equal(before["g"], opt_state(n, 8)["g"].cpu())                  # tv 0, scale 1: not rewritten
    lib.check(L.nerf_adamw_clip_step(P(st["p"].view), P(st["g"].view), P(st["m"].view), P(st["v"].view), n, 5, 1e-2, 0.9, 0.999, 1e-8, 0.0, P(ws), 0.1,
                                     0.25, None), "step")
    torch.cuda.synchronize()
    kw = dict(step=5, lr=1e-2, grad_scale=0.25, max_norm=0.1, normsq_total=raw * 0.25 ** 2, **HYP)
    assert math.sqrt(raw) * 0.25 > 1.01 * 0.1
    step_figures(before, snapshot(st), kw, "adamw_clip_step grad_scale")
    assert all(x.guards_intact() for x in st.values())


@pytest.mark.parametrize("n,mis", [(1, 0), (5, 0), (4099, 0), (4099, 1), (10007, 2), (4 * 1237, 0)])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("step,wd", [(1, 0.0), (1000, 1e-2)])
def test_adam_step(lib, n, mis, scaled, step, wd):
    L = lib.load()
    st = opt_state(n, n + step, mis=mis)
    gs = torch.tensor([0.125], device="cuda") if scaled else None
    before = snapshot(st)
    lib.check(L.nerf_adam_step(P(st["p"].view), P(st["g"].view), P(st["m"].view), P(st["v"].view), n, step, 5e-4, 0.9, 0.999, 1e-8, wd, P(gs), None), "adam")
    torch.cuda.synchronize()
    after = snapshot(st)
    assert torch.equal(after["g"], before["g"])
    step_figures(before, after, dict(step=step, lr=5e-4, weight_decay=wd, grad_scale=0.125 if scaled else 1.0, **HYP), f"adam n={n} mis={mis} step={step}")
    assert all(x.guards_intact() for x in st.values())


@pytest.mark.parametrize("n", [1, 3, 255, 257, 4099, 1 << 20 | 1])
def test_f32_to_f16_rounds_like_half(lib, n):
    L = lib.load()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * torch.pow(10.0, torch.randint(-9, 6, (n,), generator=gen).float())
    special = torch.tensor([65504.0, 65519.9, 65520.0, 1e6, -1e6, 6.1e-5, 5.96e-8, 2.98e-8, 2.9e-8, -0.0, 0.0, 6.0975e-5, 1.0009765625, 1.00048828125])
    x[:min(n, special.numel())] = special[:n]
    src, dst = Guarded(x), Guarded(torch.zeros(n, dtype=torch.float16), fill=77.0)
    lib.check(L.nerf_f32_to_f16(P(src.view), P(dst.view), n, None), "f32_to_f16")
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu().view(torch.int16), x.half().view(torch.int16))
    assert torch.equal(src.cpu(), x) and src.guards_intact() and dst.guards_intact()
