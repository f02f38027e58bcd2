"""The keyword wrappers of the step's tail in ops.py (tv_normsq_codes, adamw_clip_step_tv and their _piece forms) against the raw
ctypes calls they replaced at the engines' call sites: the same launches with the same arguments, so every output is the same
bits -- params, both moments, the fp16 copy, the TV sign codes and normsq[0], compared as integers.

Shapes: the smallest that reach every branch the wrappers choose between -- one (weight, elements) pair against the five-tuple of
two ranges, ``tv=None`` against a pair, ``lr_split`` given or not, ``codes`` / ``shadow_f16`` given or not, a storing and an
accumulating first pass, the table kernel (aligned, n % 4 == 0) and the generic one (n = 10007, misaligned by one element).

The entry refuses an lr_split that is neither a multiple of 4 nor past the end, so the two-range case of n = 4 * 1024 puts it on the
last CHUNK (n - 4); the last ELEMENT, as Part 4's network buffer has it (30144 of 30145), is in the no-TV case, whose n is 4 k + 1.
"""
import pytest
import torch

from test_gpu_step_tail import Guarded, P, lib, opt_state  # noqa: F401  (lib: the module's fixture)

pytestmark = pytest.mark.gpu
STEP, LR, WD, MAX_NORM, GS = 3, 1e-2, 1e-2, 0.05, 0.5


def buffers(lib, n, mis, seed, kind="stairs", sets=2):
    """identical sets of state, fp16 copy, codes (behind 16 spare bytes, as the pieces need) and norm workspace"""
    out = []
    for _ in range(sets):
        st = opt_state(n, seed, kind, mis)
        st["h"] = Guarded(torch.zeros(n, dtype=torch.float16), 0 if mis == 0 else 4, fill=77.0)
        st["c"] = Guarded(torch.zeros(16 + (n + 3) // 4, dtype=torch.uint8))
        st["ws"] = torch.zeros(lib.NORMSQ_WS_FLOATS, device="cuda")
        st["ws"][0] = 3.0e7                        # a storing first pass overwrites it
        out.append(st)
    return out


def same_bits(raw, new, keys="pgmvhc", normsq=True):
    torch.cuda.synchronize()
    ints = {torch.float32: torch.int32, torch.float16: torch.int16, torch.uint8: torch.uint8}
    for k in keys:
        a, b = raw[k].full, new[k].full          # guards included: neither form writes outside its view
        assert torch.equal(a.view(ints[a.dtype]), b.view(ints[b.dtype])), k
        assert raw[k].guards_intact() and new[k].guards_intact(), k
    if normsq:
        assert torch.equal(raw["ws"][:1].view(torch.int32), new["ws"][:1].view(torch.int32)), "normsq[0]"
    else:           # partial sums added in another order: equal to rounding
        assert abs(float(new["ws"][0]) - float(raw["ws"][0])) <= 1e-5 * float(raw["ws"][0]), "normsq[0]"
    assert 0.0 < float(new["ws"][0]) < 1.0e7


V = lambda st, *keys: [st[k].view for k in keys]


@pytest.mark.parametrize("n,mis,n_tables,tv_w", [(4 * 1237, 0, 1, 0.6), (3 * 1024, 0, 3, 0.7), (10007, 1, 1, 0.6)])
def test_one_tv_weight(lib, n, mis, n_tables, tv_w):
    """one table with TV and the fp16 copy; three equal tables; the generic kernels (misaligned by one element)"""
    from project_nerf_amd import ops
    L, seg = lib.load(), n // n_tables
    raw, new = buffers(lib, n, mis, 5)
    p, g, m, v, h, c, ws = V(raw, "p", "g", "m", "v", "h", "c") + [raw["ws"]]
    lib.check(L.nerf_tv_normsq_codes(P(p), P(g), n, n_tables, tv_w, GS, P(ws), 0, P(c[16:]), None), "raw")
    lib.check(L.nerf_adamw_clip_step_tv(P(p), P(g), P(m), P(v), n, STEP, LR, 0.9, 0.999, 1e-8, WD, P(ws), MAX_NORM, GS, P(c[16:]), n, tv_w, seg,
                                        0.0, 0, 0, 0.0, P(h), None), "raw")
    p, g, m, v, h, c, ws = V(new, "p", "g", "m", "v", "h", "c") + [new["ws"]]
    ops.tv_normsq_codes(p, g, n, ws, n_tables=n_tables, tv_weight=tv_w, grad_scale=GS, codes=c[16:])
    ops.adamw_clip_step_tv(p, g, m, v, n, STEP, LR, ws, weight_decay=WD, max_norm=MAX_NORM, grad_scale=GS, codes=c[16:], tv=(tv_w, seg),
                           shadow_f16=h)
    same_bits(raw, new)


def test_two_ranges_with_their_own_weights_and_a_second_rate(lib):
    """Part 4's tables: three deformation grids and the canonical one under ONE norm, a TV weight per range"""
    from project_nerf_amd import ops
    L, n, split, w_lo, w_hi, lr_hi = lib.load(), 4 * 1024, 3 * 1024, 0.8, 0.05, 4e-3
    raw, new = buffers(lib, n, 0, 6)
    p, g, m, v, h, c, ws = V(raw, "p", "g", "m", "v", "h", "c") + [raw["ws"]]
    lib.check(L.nerf_tv_normsq_codes(P(p), P(g), split, 3, w_lo, GS, P(ws), 0, P(c[16:]), None), "raw")
    lib.check(L.nerf_tv_normsq_codes(P(p[split:]), P(g[split:]), n - split, 1, w_hi, GS, P(ws), 1, P(c[16 + split // 4:]), None), "raw")
    lib.check(L.nerf_adamw_clip_step_tv(P(p), P(g), P(m), P(v), n, STEP, LR, 0.9, 0.999, 1e-8, WD, P(ws), MAX_NORM, GS, P(c[16:]), split, w_lo, 1024,
                                        w_hi, n - split, n - 4, lr_hi, P(h), None), "raw")
    p, g, m, v, h, c, ws = V(new, "p", "g", "m", "v", "h", "c") + [new["ws"]]
    ops.tv_normsq_codes(p, g, split, ws, n_tables=3, tv_weight=w_lo, grad_scale=GS, codes=c[16:])
    ops.tv_normsq_codes(p[split:], g[split:], n - split, ws, tv_weight=w_hi, grad_scale=GS, accumulate=True, codes=c[16 + split // 4:])
    ops.adamw_clip_step_tv(p, g, m, v, n, STEP, LR, ws, weight_decay=WD, max_norm=MAX_NORM, grad_scale=GS, codes=c[16:],
                           tv=(split, w_lo, 1024, w_hi, n - split), lr_split=(n - 4, lr_hi), shadow_f16=h)
    same_bits(raw, new)


def test_network_buffer_without_a_tv_term(lib):
    """codes=None, tv=None, no fp16 copy, the last element at its own rate (Part 4's displacement_scale)"""
    from project_nerf_amd import ops
    L, n, lr_hi = lib.load(), 4 * 300 + 1, 4e-3
    raw, new = buffers(lib, n, 0, 7, "random")
    p, g, m, v, ws = V(raw, "p", "g", "m", "v") + [raw["ws"]]
    lib.check(L.nerf_tv_normsq_codes(P(p), P(g), n, 1, 0.0, GS, P(ws), 0, None, None), "raw")
    lib.check(L.nerf_adamw_clip_step_tv(P(p), P(g), P(m), P(v), n, STEP, LR, 0.9, 0.999, 1e-8, WD, P(ws), MAX_NORM, GS, None, 0, 0.0, 0, 0.0, 0,
                                        n - 1, lr_hi, None, None), "raw")
    p, g, m, v, ws = V(new, "p", "g", "m", "v") + [new["ws"]]
    ops.tv_normsq_codes(p, g, n, ws, grad_scale=GS)
    ops.adamw_clip_step_tv(p, g, m, v, n, STEP, LR, ws, weight_decay=WD, max_norm=MAX_NORM, grad_scale=GS, lr_split=(n - 1, lr_hi))
    same_bits(raw, new)                            # h, c: untouched by both


def test_pieces_against_the_raw_pieces_and_the_whole_table(lib):
    """one table in 3 pieces (halo bits as sharded.py sets them, every piece's codes in ONE buffer) through the _piece wrappers:
    against the raw _piece calls bit for bit, and against the whole-table raw calls -- there the norm is summed in another order,
    and without a clip it does not reach the step"""
    from project_nerf_amd import ops
    L, n, tv_w, cuts = lib.load(), 4 * 1237, 0.6, [0, 4 * 400, 4 * 401, 4 * 1237]
    whole, raw, new = buffers(lib, n, 0, 8, sets=3)
    p, g, m, v, h, c, ws = V(whole, "p", "g", "m", "v", "h", "c") + [whole["ws"]]
    lib.check(L.nerf_tv_normsq_codes(P(p), P(g), n, 1, tv_w, GS, P(ws), 0, P(c[16:]), None), "whole")
    lib.check(L.nerf_adamw_clip_step_tv(P(p), P(g), P(m), P(v), n, STEP, LR, 0.9, 0.999, 1e-8, WD, P(ws), 0.0, GS, P(c[16:]), n, tv_w, n,
                                        0.0, 0, 0, 0.0, P(h), None), "whole")
    spans = [(a, b - a, (1 if a > 0 else 0) | (2 if b < n else 0)) for a, b in zip(cuts[:-1], cuts[1:])]
    p, g, m, v, h, c, ws = V(raw, "p", "g", "m", "v", "h", "c") + [raw["ws"]]
    for i, (a, cnt, halo) in enumerate(spans):
        lib.check(L.nerf_tv_normsq_codes_piece(P(p[a:]), P(g[a:]), cnt, n, halo, tv_w, GS, P(ws), 0 if i == 0 else 1, P(c[16 + a // 4:]), None), "raw")
    for a, cnt, halo in spans:
        lib.check(L.nerf_adamw_clip_step_tv_piece(P(p[a:]), P(g[a:]), P(m[a:]), P(v[a:]), cnt, STEP, LR, 0.9, 0.999, 1e-8, WD, P(ws), 0.0, GS,
                                                  P(c[16 + a // 4:]), tv_w, n, halo & 1, P(h[a:]), None), "raw")
    p, g, m, v, h, c, ws = V(new, "p", "g", "m", "v", "h", "c") + [new["ws"]]
    for i, (a, cnt, halo) in enumerate(spans):
        ops.tv_normsq_codes_piece(p[a:], g[a:], cnt, ws, table_elems=n, halo=halo, tv_weight=tv_w, grad_scale=GS, accumulate=i > 0,
                                  codes=c[16 + a // 4:])
    for a, cnt, halo in spans:
        ops.adamw_clip_step_tv_piece(p[a:], g[a:], m[a:], v[a:], cnt, STEP, LR, ws, weight_decay=WD, max_norm=0.0, grad_scale=GS, table_elems=n,
                                     halo_lo=halo & 1, tv_weight=tv_w, codes=c[16 + a // 4:], shadow_f16=h[a:])
    same_bits(raw, new)
    same_bits(whole, new, normsq=False)
