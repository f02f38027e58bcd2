"""The fragment images of the resident-weight tiny-MLP chains (csrc/resident_chain.h::pack_fragments behind nerf_imlp_pack,
nerf_p4_pack, nerf_p3_deform_pack and nerf_imlp_shape_pack) against a host restatement, byte for byte.

Every step's dense A [32 mt, 16 (ks_acc + ks_nat)] is rebuilt here from slices of the parameter vector (transposed for the
transposed steps, zero in the pads), permuted by the column order of mlp_plan.h::frag_column and rounded with torch: to fp16 for
the forward steps of Part 4 and Part 3, to bf16 everywhere else.  The step tables below are data of this test, not read from the
library.  No sample axis: one launch per engine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
P = lambda t: t.data_ptr()


def mat(v, off, rows, ld):
    return v[off:off + rows * ld].view(rows, ld)


# A step: (mt, ks_acc, ks_nat, frag0, fp16, acc pieces, nat pieces); a piece: (first column, matrix of the vector -> [rows, cols])
def imlp_steps():
    SW1, SW2, CW1, CW2, CW3 = 0, 2048, 3072, 6144, 10240
    s1 = lambda v: mat(v, SW1, 64, 32)
    s2 = lambda v: mat(v, SW2, 16, 64)
    c1 = lambda v: mat(v, CW1, 64, 48)
    c2 = lambda v: mat(v, CW2, 64, 64)
    c3 = lambda v: mat(v, CW3, 16, 64)
    return [
        (2, 0, 2, 0, False, [], [(0, s1)]),
        (1, 4, 0, 4, False, [(0, s2)], []),
        (2, 1, 2, 8, False, [(0, lambda v: c1(v)[:, :16])], [(0, lambda v: c1(v)[:, 16:43])]),
        (2, 4, 0, 14, False, [(0, c2)], []),
        (1, 4, 0, 22, False, [(0, lambda v: c3(v)[:3])], []),
        (2, 0, 1, 26, False, [], [(0, lambda v: c3(v)[:3].T)]),
        (2, 4, 0, 28, False, [(0, lambda v: c2(v).T)], []),
        (1, 4, 0, 36, False, [(0, lambda v: c1(v)[:, :16].T)], []),
        (2, 1, 0, 40, False, [(0, lambda v: s2(v).T)], []),
        (1, 4, 0, 42, False, [(0, lambda v: s1(v).T)], []),
    ]


def p4_steps():
    T1W, T1b, T2W, D1, D2, D3 = 0, 1344, 1408, 5568, 11712, 15808
    S1, S2, C1, C2, C3 = 16832, 20928, 21952, 25024, 29120
    t1 = lambda v: mat(v, T1W, 64, 21)
    t1b = lambda v: mat(v, T1b, 64, 1)
    t2 = lambda v: mat(v, T2W, 64, 64)
    d1 = lambda v: mat(v, D1, 64, 96)
    d2 = lambda v: mat(v, D2, 64, 64)
    d3 = lambda v: mat(v, D3, 16, 64)
    s1 = lambda v: mat(v, S1, 64, 64)
    s2 = lambda v: mat(v, S2, 16, 64)
    c1 = lambda v: mat(v, C1, 64, 48)
    c2 = lambda v: mat(v, C2, 64, 64)
    c3 = lambda v: mat(v, C3, 16, 64)
    return [
        (2, 0, 2, 0, True, [], [(0, t1), (21, t1b)]),                                        # T1: the bias rides on code column 21
        (2, 4, 0, 4, True, [(0, t2)], []),                                                   # T2
        (2, 4, 2, 12, True, [(0, lambda v: d1(v)[:, 24:88])], [(0, lambda v: d1(v)[:, :24])]),   # D1: [tm | df]
        (2, 4, 0, 24, True, [(0, d2)], []),                                                  # D2
        (1, 4, 0, 32, True, [(0, lambda v: d3(v)[:3])], []),                                 # D3
        (2, 0, 1, 36, False, [], [(0, lambda v: d3(v)[:3].T)]),                              # D3t
        (2, 4, 0, 38, False, [(0, lambda v: d2(v).T)], []),                                  # D2t
        (2, 4, 0, 46, False, [(0, lambda v: d1(v)[:, 24:88].T)], []),                        # D1tT
        (1, 4, 0, 54, False, [(0, lambda v: d1(v)[:, :24].T)], []),                          # D1tH
        (2, 4, 0, 58, False, [(0, lambda v: t2(v).T)], []),                                  # T2t
        (2, 0, 4, 66, True, [], [(0, lambda v: s1(v)[:, :53])]),                             # S1: [hash 32 | tcode 21]
        (1, 4, 0, 74, True, [(0, s2)], []),                                                  # S2
        (2, 1, 2, 78, True, [(0, lambda v: c1(v)[:, :16])], [(0, lambda v: c1(v)[:, 16:43])]),   # C1
        (2, 4, 0, 84, True, [(0, c2)], []),                                                  # C2
        (1, 4, 0, 92, True, [(0, lambda v: c3(v)[:3])], []),                                 # C3
        (2, 0, 1, 96, False, [], [(0, lambda v: c3(v)[:3].T)]),                              # C3t
        (2, 4, 0, 98, False, [(0, lambda v: c2(v).T)], []),                                  # C2t
        (1, 4, 0, 106, False, [(0, lambda v: c1(v)[:, :16].T)], []),                         # C1t
        (2, 1, 0, 110, False, [(0, lambda v: s2(v).T)], []),                                 # S2t
        (1, 4, 0, 112, False, [(0, lambda v: s1(v)[:, :32].T)], []),                         # S1t: hash rows only
    ]


def p3_steps():
    W1, B1, W2, W3, W4 = 0, 10752, 10880, 27392, 43904
    w1 = lambda v: mat(v, W1, 128, 84)
    b1 = lambda v: mat(v, B1, 128, 1)
    w2 = lambda v: mat(v, W2, 128, 128)
    w3 = lambda v: mat(v, W3, 128, 128)
    w4 = lambda v: mat(v, W4, 3, 128)
    return [
        (4, 0, 6, 0, True, [], [(0, w1), (84, b1)]),                                         # F1: b1 rides on code column 84
        (4, 8, 0, 24, True, [(0, w2)], []),
        (4, 8, 0, 56, True, [(0, w3)], []),
        (1, 8, 0, 88, True, [(0, w4)], []),
        (4, 0, 1, 96, False, [], [(0, lambda v: w4(v).T)]),
        (4, 8, 0, 100, False, [(0, lambda v: w3(v).T)], []),
        (4, 8, 0, 132, False, [(0, lambda v: w2(v).T)], []),
    ]


def p4_bias(v):
    return v[5504:5568]                                                                      # T2b


def p3_bias(v):
    return torch.cat([v[27264:27392], v[43776:43904], v[44288:44291], torch.zeros(512 - 259)])   # b2 | b3 | b4 | 0


ENGINES = {
    "imlp": dict(pack="nerf_imlp_pack", bytes="nerf_imlp_packed_bytes", n_params=11264, steps=imlp_steps, frags=46, bias=None),
    "p4": dict(pack="nerf_p4_pack", bytes="nerf_p4_packed_bytes", n_params=30145, steps=p4_steps, frags=116, bias=p4_bias),
    "p3": dict(pack="nerf_p3_deform_pack", bytes="nerf_p3_deform_packed_bytes", n_params=44291, steps=p3_steps, frags=164, bias=p3_bias),
}


def seeded_vector(n):
    """weights of a trained network's size, plus values that fp16 and bf16 round to different things: past fp16's largest finite
    value (inf / finite), in its subnormal range and below it (0 / non-zero), and eleven-bit mantissas that bf16 cuts"""
    g = torch.Generator().manual_seed(20240607 + n)
    v = torch.randn(n, generator=g) * 0.4
    special = torch.tensor([70000.0, -1.0e5, 3.0e-6, -4.5e-7, 1.0e-30, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10), 0.1, 65520.0, 0.0])
    at = torch.randperm(n, generator=g)[:n // 8]
    v[at] = special[torch.arange(at.numel()) % special.numel()]
    return v


def frag_column(ks_rel, h, j, nat):
    return 16 * ks_rel + 8 * h + j if nat else 32 * (ks_rel >> 1) + 16 * (ks_rel & 1) + 8 * (j >> 2) + 4 * h + (j & 3)


def dense(v, mt, ks, pieces):
    A = torch.zeros(32 * mt, 16 * ks)
    for col0, f in pieces:
        m = f(v)
        assert m.shape[0] <= A.shape[0] and col0 + m.shape[1] <= A.shape[1], (tuple(m.shape), col0, tuple(A.shape))
        A[:m.shape[0], col0:col0 + m.shape[1]] = m
    return A


def host_image(v, steps, n_frags):
    """[n_frags, 64 lanes, 8] int16: the bit patterns the pack kernels store"""
    out = torch.zeros(n_frags, 64, 8, dtype=torch.int16)
    lane = np.arange(64)
    row, h = lane & 31, lane >> 5
    covered = 0
    for mt, ks_acc, ks_nat, frag0, fp16, acc_pieces, nat_pieces in steps:
        assert frag0 == covered, "the step table leaves no gap"
        parts = [dense(v, mt, ks_acc, acc_pieces), dense(v, mt, ks_nat, nat_pieces)]
        ksn = ks_acc + ks_nat
        for m in range(mt):
            for ks in range(ksn):
                nat = ks >= ks_acc
                cols = np.stack([frag_column(ks - ks_acc if nat else ks, h, j, nat) for j in range(8)], axis=1)     # [64, 8]
                vals = parts[1 if nat else 0][torch.from_numpy(32 * m + row)[:, None], torch.from_numpy(cols)]
                out[frag0 + m * ksn + ks] = (vals.to(torch.float16) if fp16 else vals.to(torch.bfloat16)).view(torch.int16)
        covered += mt * ksn
    assert covered == n_frags
    return out


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def images(lib):
    """engine -> (parameter vector, packed bytes from the library, host image, host bias table or None)"""
    from project_nerf_amd import ops
    out = {}
    for name, e in ENGINES.items():
        v = seeded_vector(e["n_params"])
        packed = torch.full((getattr(lib, e["bytes"])(),), 0xA5, device="cuda", dtype=torch.uint8)
        vd = v.cuda()
        assert getattr(lib, e["pack"])(P(vd), P(packed), ops._stream()) == 0
        torch.cuda.synchronize()
        out[name] = (v, packed.cpu(), host_image(v, e["steps"](), e["frags"]), None if e["bias"] is None else e["bias"](v))
    return out


@pytest.mark.parametrize("engine", list(ENGINES))
def test_packed_fragments_and_bias_table_match_the_host_image(images, engine):
    v, packed, want, bias = images[engine]
    n_frags = ENGINES[engine]["frags"]
    got = packed[:n_frags * 1024].view(torch.int16).view(n_frags, 64, 8)
    bad = (got != want).any(dim=2).any(dim=1).nonzero().flatten().tolist()
    assert torch.equal(got, want), f"{engine}: fragments {bad[:16]} differ ({len(bad)} of {n_frags})"
    if bias is None:
        assert packed.numel() == n_frags * 1024
    else:
        tail = packed[n_frags * 1024:]
        assert tail.numel() == bias.numel() * 4
        assert torch.equal(tail.view(torch.float32), bias), f"{engine}: bias table differs"


def test_shape_pack_at_the_default_shape_is_the_instant_pack(lib, images):
    """(16, 64, 4): both step tables give frag0 = 0 4 8 14 22 | 26 28 36 40 42 and the same source map"""
    from project_nerf_amd import ops
    v, packed, want, _ = images["imlp"]
    assert [s[3] for s in imlp_steps()] == [0, 4, 8, 14, 22, 26, 28, 36, 40, 42]
    assert lib.nerf_imlp_shape_param_count(16, 64, 4) == v.numel()
    assert lib.nerf_imlp_shape_packed_bytes(16, 64, 4) == packed.numel()
    shaped = torch.full((packed.numel(),), 0x5A, device="cuda", dtype=torch.uint8)
    vd = v.cuda()
    assert lib.nerf_imlp_shape_pack(P(vd), 16, 64, 4, P(shaped), ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(shaped.cpu(), packed)
    assert torch.equal(shaped.cpu().view(torch.int16).view(46, 64, 8), want)
