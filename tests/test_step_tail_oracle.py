"""Pins the float64 references of the step tail (oracle.composite_mse_reg, oracle.tv_clip_adamw) that
tests/test_gpu_step_tail.py compares the HIP kernels with.  CPU only.

* tv_clip_adamw against torch itself in float64: autograd of tv_weight * mean|t[1:] - t[:-1]| per table,
  torch.nn.utils.clip_grad_norm_ over all tables at once, torch.optim.AdamW from given moments.  Both sides are float64
  restatements of the same formula in a different order of operations: 1e-12 relative.
* composite_mse_reg against the committed reference goldens g5_composite_* (fp32 results of the reference's own
  compositing and autograd).  The goldens' cotangent of the pixel is folded into the target
  (target = pixel - g_rgb_map / (2 loss_weight), so d loss / d pixel = g_rgb_map); their cotangents of depth and
  opacity, which the fused step does not have, are removed from the golden d_sigma with the float64 autograd of
  oracle.composite (itself pinned on the same goldens by test_oracle_golden).  The goldens are fp32: the bound is the
  project's fp32 one for this operation (d_rgb rtol 1e-5, d_sigma 2e-5 of the ray's maximum, pixel rtol 1e-6 / atol 1e-7).
"""
import math

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import nerf_oracle as O

T = torch.from_numpy
F64 = torch.float64


def staircase(n, gen):
    """runs of equal values of lengths 1..9: ties on every position"""
    vals, k = [], 0
    while len(vals) < n:
        vals += [float(torch.randn((), generator=gen))] * (1 + k % 9)
        k += 1
    return torch.tensor(vals[:n])


@pytest.mark.parametrize("sizes", [(7,), (1,), (2,), (12, 12, 12), (8, 8, 8, 8), (5, 16, 3)])
@pytest.mark.parametrize("step,max_norm,wd,grad_scale", [(1, 0.0, 0.0, 1.0), (2, 0.05, 1e-2, 0.25), (1000, 1e4, 1e-5, 3.0)])
def test_tv_clip_adamw_equals_torch_adamw_clip_and_autograd(sizes, step, max_norm, wd, grad_scale):
    gen = torch.Generator().manual_seed(sum(sizes) + step)
    n = sum(sizes)
    p0 = staircase(n, gen) if step == 2 else torch.randn(n, generator=gen)
    g0 = torch.randn(n, generator=gen) * 1e-2
    m0 = torch.randn(n, generator=gen) * 1e-2
    v0 = torch.rand(n, generator=gen) * 1e-4
    weights = [0.3, 0.0, 1.7, 0.02][:len(sizes)]
    lr, lr_hi = 1e-2, 3e-3
    tables, off = [], 0
    for sz, w in zip(sizes, weights):
        tables.append((off, sz, w))
        off += sz
    lr_split = sizes[0] if len(sizes) > 1 else 0
    out = O.tv_clip_adamw(p0, g0, m0, v0, step, lr, weight_decay=wd, tables=tables, grad_scale=grad_scale, max_norm=max_norm,
                          lr_split=lr_split, lr_hi=lr_hi)
    # torch: one parameter per table, the first table in its own group (lr), the rest in another (lr_hi)
    params = [torch.nn.Parameter(p0[o:o + sz].to(F64).clone()) for o, sz, _ in tables]
    groups = [{"params": params[:1], "lr": lr}] + ([{"params": params[1:], "lr": lr_hi}] if len(params) > 1 else [])
    opt = torch.optim.AdamW(groups, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    tv = sum(w * (q[1:] - q[:-1]).abs().mean() for q, (_, sz, w) in zip(params, tables) if sz > 1 and w != 0.0)
    if torch.is_tensor(tv):
        tv.backward()
    for q, (o, sz, _) in zip(params, tables):
        data = g0[o:o + sz].to(F64) * grad_scale
        q.grad = data if q.grad is None else q.grad + data
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0[o:o + sz].to(F64).clone(),
                        "exp_avg_sq": v0[o:o + sz].to(F64).clone()}
    grad = torch.cat([q.grad for q in params])
    np.testing.assert_allclose(out["grad"].numpy(), grad.numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(out["normsq"], float((grad ** 2).sum()), rtol=1e-12)
    if max_norm > 0.0:
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        assert (out["coef"] < 1.0) == (max_norm < math.sqrt(out["normsq"]))
    opt.step()
    np.testing.assert_allclose(out["p"].numpy(), torch.cat([q.detach() for q in params]).numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(out["m"].numpy(), torch.cat([opt.state[q]["exp_avg"] for q in params]).numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(out["v"].numpy(), torch.cat([opt.state[q]["exp_avg_sq"] for q in params]).numpy(), rtol=1e-12, atol=1e-300)
    # the sign codes, restated element by element
    codes = out["codes"].numpy()
    assert codes.shape == ((n + 3) // 4,)
    for o, sz, _ in tables:
        for i in range(sz):
            s = 0 if i == sz - 1 else int(np.sign(float(p0[o + i + 1]) - float(p0[o + i])))
            assert (codes[(o + i) // 4] >> (2 * ((o + i) % 4))) & 3 == 1 + s
    if n % 4:
        assert codes[-1] >> (2 * (n % 4)) == 0


def test_tv_clip_adamw_under_a_shared_norm():
    """normsq_total: the clip of one group under the norm of several"""
    gen = torch.Generator().manual_seed(3)
    p, g, m, v = (torch.randn(16, generator=gen) for _ in range(4))
    v = v.abs()
    own = O.tv_clip_adamw(p, g, m, v, 3, 1e-2, max_norm=0.5)
    shared = O.tv_clip_adamw(p, g, m, v, 3, 1e-2, max_norm=0.5, normsq_total=own["normsq"] * 4.0)
    assert own["coef"] < 1.0
    np.testing.assert_allclose(shared["coef"], 0.5 / (2.0 * math.sqrt(own["normsq"]) + 1e-6), rtol=1e-14)
    np.testing.assert_allclose(shared["m"].numpy(), (0.9 * m.double() + 0.1 * g.double() * shared["coef"]).numpy(), rtol=1e-12)


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("tag", ["none", "vec", "ray"])
def test_composite_mse_reg_vs_reference_golden(S, tag):
    g = golden(f"g5_composite_S{S}_{tag}")
    bg = None if g["bg"].size == 0 else T(g["bg"])
    R = g["z"].shape[0]
    lw = 1.0 / (3 * R)
    target = T(g["out_rgb"]).to(F64) - T(g["g_rgb_map"]).to(F64) / (2.0 * lw)
    out = O.composite_mse_reg(T(g["rgb"]), T(g["sigma"]), T(g["z"]), T(g["rays_d"]), bg, target, lw)
    np.testing.assert_allclose(out["pixel"].numpy(), g["out_rgb"], rtol=1e-6, atol=1e-7)
    assert out["pixel"].dtype == F64 and out["d_sigma"].dtype == F64
    # the gradient of the pixel equals the golden cotangent only as far as the float64 pixel equals the fp32 one
    # (|g_rgb_map| ~ 1, the pixels differ by ~1e-7: 2 lw dpixel ~ 1e-9 relative to 1): inside the bounds below
    np.testing.assert_allclose(out["d_rgb"].view(R, S, 3).numpy(), g["d_rgb"], rtol=1e-5, atol=1e-7)
    sig = T(g["sigma"]).to(F64).requires_grad_(True)
    _, dep, acc = O.composite(T(g["rgb"]).to(F64), sig, T(g["z"]).to(F64), T(g["rays_d"]).to(F64), None if bg is None else bg.to(F64))
    ((dep * T(g["g_depth"]).to(F64)).sum() + (acc * T(g["g_acc"]).to(F64)).sum()).backward()
    ref = g["d_sigma"].astype(np.float64) - sig.grad.numpy()
    got, gold = out["d_sigma"].view(R, S).numpy(), np.abs(g["d_sigma"]).astype(np.float64)
    # all samples but the far one, scaled by their ray's maximum over them
    assert np.max(np.abs(got[:, :-1] - ref[:, :-1]) / (gold[:, :-1].max(axis=1, keepdims=True) + 1e-300)) < 2e-5
    # the far sample (interval 1e10: it would hide every other sample of its ray in a common scale) by its own relative
    # error.  Its derivative is proportional to the transmittance in front of it, a product of q_j = 1 - alpha_j + 1e-10
    # whose fp32 value carries an absolute rounding error of up to 2^-24 each (alpha_j = 1 - e_j rounds at the scale of 1):
    # the fp32 golden's relative error there is up to sum_j 2^-24 / q_j, which is all it can pin on a saturated ray.
    # 1.2e-38 (the smallest normal fp32): the golden's underflow.
    z, d = T(g["z"]).to(F64), T(g["rays_d"]).to(F64)
    q = torch.exp(-T(g["sigma"]).to(F64)[:, :-1] * (z[:, 1:] - z[:, :-1]) * d.norm(dim=-1, keepdim=True)) + 1e-10
    far_rel = 2e-5 + (2.0 ** -24 / q).sum(dim=1).numpy()
    assert np.all(np.abs(got[:, -1] - ref[:, -1]) <= far_rel * gold[:, -1] + 1.2e-38)
    assert np.sum(far_rel < 1e-4) >= R // 8                 # the far-sample check binds on some rays of every golden
    assert out["reg"] == 0.0 and out["d_extra"] is None and bool(out["mapped"].all())
    np.testing.assert_allclose(out["loss"], float(lw * ((T(g["g_rgb_map"]).to(F64) / (2.0 * lw)) ** 2).sum()), rtol=1e-5)


def test_composite_mse_reg_slot_map_equals_zero_filled_dense_and_regulariser_by_hand():
    gen = torch.Generator().manual_seed(11)
    R, S = 5, 9
    z = torch.sort(torch.rand(R, S, generator=gen) * 4 + 2, dim=-1).values
    d = torch.randn(R, 3, generator=gen)
    active = torch.rand(R, S, generator=gen) < 0.4
    active[0] = False
    active[1] = True
    n = int(active.sum())
    perm = torch.randperm(n + 3, generator=gen)[:n]              # three rows of the compact arrays nothing maps to
    slots = torch.full((R, S), -1, dtype=torch.int32)
    slots[active] = perm.to(torch.int32)
    rgb, sig, ext = torch.rand(n + 3, 3, generator=gen), torch.rand(n + 3, generator=gen) * 2, torch.randn(n + 3, 3, generator=gen)
    target, bg = torch.rand(R, 3, generator=gen), torch.rand(1, 3, generator=gen)
    out = O.composite_mse_reg(rgb, sig, z, d, bg, target, 0.3, ext, 0.7, slots)
    dense = [torch.zeros(R * S, *t.shape[1:]) for t in (rgb, sig, ext)]
    for full, compact in zip(dense, (rgb, sig, ext)):
        full[active.reshape(-1)] = compact[perm]
    ref = O.composite_mse_reg(dense[0], dense[1], z, d, bg, target, 0.3, dense[2], 0.7)
    for k in ("pixel", "m"):
        assert torch.equal(out[k], ref[k])
    assert out["loss"] == ref["loss"] and out["reg"] == ref["reg"]
    assert int(out["mapped"].sum()) == n and not bool(out["mapped"][[i for i in range(n + 3) if i not in set(perm.tolist())]].any())
    for k in ("d_rgb", "d_sigma", "d_extra"):
        assert torch.equal(out[k][perm], ref[k][active.reshape(-1)])
        assert float(out[k][~out["mapped"]].abs().max()) == 0.0
    # m, reg and d_extra by hand from the weights
    _, _, _, w = O.composite(dense[0].view(R, S, 3).double(), dense[1].view(R, S).double(), z.double(), d.double(), bg.double(), True)
    m = (w[..., None] * dense[2].view(R, S, 3).double()).sum(1)
    np.testing.assert_allclose(out["m"].numpy(), m.numpy(), rtol=1e-14)
    np.testing.assert_allclose(out["reg"], 0.7 * float((m ** 2).sum()), rtol=1e-14)
    np.testing.assert_allclose(ref["d_extra"].view(R, S, 3).numpy(), (w[..., None] * (2 * 0.7 * m)[:, None, :]).numpy(), rtol=1e-12, atol=1e-300)
    assert float(out["pixel"][0].sub(bg[0].double()).abs().max()) == 0.0          # the ray with nothing active shows the background
