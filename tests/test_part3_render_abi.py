"""Host-side checks of nerf_p3_render_* (the evaluation launch chain of Part 3 with a hash-grid canonical field): the workspace size
query against the layout include/nerf_hip.h documents, piece by piece, and the argument validation, which returns before anything is
launched -- no GPU needed."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b"nerf_p3_render_rays_fwd"


@pytest.fixture(scope="module")
def lib():
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("nerf_build", os.path.join(ROOT, "project-nerf_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    return _lib.load()


def up256(b):
    return (b + 255) // 256 * 256


def pieces(chunk, S):
    """the layout of include/nerf_hip.h restated: header, z, slots, pts, dirs, operands (x_c [roundup(n, 128), 3] fp32, then the fp16
    canonical image [roundup(n, 128), 32]), rgb, sigma"""
    n = chunk * S
    n_pad = (n + 127) // 128 * 128
    return [("count", 256), ("z", up256(n * 4)), ("slots", up256(n * 4)), ("pts", up256(n * 12)), ("dirs", up256(n * 12)),
            ("operands", up256(n_pad * 12 + n_pad * 64)), ("rgb", up256(n * 12)), ("sigma", up256(n * 4))]


def documented_bytes(chunk, S):
    return sum(b for _, b in pieces(chunk, S))


def test_symbols_are_exported_and_bound(lib):
    from project_nerf_amd import _lib, ops
    for name in ("nerf_p3_render_rays_fwd", "nerf_p3_render_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert callable(ops.p3_render_rays_fwd) and callable(ops.p3_render_workspace_bytes)
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert "int nerf_p3_render_rays_fwd(" in header
    assert "size_t nerf_p3_render_workspace_bytes(int64_t chunk_rays, int n_samples);" in header
    assert len(_lib.PROTOTYPES["nerf_p3_render_rays_fwd"][1]) == 29          # the declaration's arguments, time_dev among them


def test_workspace_size_query(lib):
    from project_nerf_amd import ops
    q = lib.nerf_p3_render_workspace_bytes
    for chunk, S in ((0, 128), (-1, 128), (5, 0), (5, -3), (0, 0), (-4, -4)):
        assert q(chunk, S) == 0
    for chunk, S in ((1, 2), (1, 127), (1, 128), (3, 43), (5, 64), (13, 64), (40, 128), (4096, 64), (65536, 64)):
        assert q(chunk, S) == documented_bytes(chunk, S), (chunk, S, pieces(chunk, S))
        assert q(chunk, S) % 256 == 0
    # 4096 x 64 = 2^18 samples, every piece a multiple of 256 already: 256 + (4 + 4 + 12 + 12 + 76 + 12 + 4) = 124 bytes per sample
    assert dict(pieces(4096, 64))["operands"] == 2 ** 18 * 76
    assert q(4096, 64) == 256 + 124 * 2 ** 18 == 32506112
    assert ops.p3_render_workspace_bytes(4096, 64) == 32506112
    # the operand piece is what nerf_p3_grid_update keeps per slab; the Instant chain's piece is the image alone
    assert q(4096, 64) - lib.nerf_instant_render_workspace_bytes(4096, 64) == 2 ** 18 * 12
    assert dict(pieces(4096, 64))["operands"] == lib.nerf_p3_grid_update_workspace_bytes(2 ** 18)
    # the two training layouts the loop lays out per chunk are an order of magnitude larger
    assert lib.nerf_p4_workspace_bytes(2 ** 18) > 8 * q(4096, 64)
    # a row count that is no multiple of 128: the operand piece is padded, the others are not
    assert dict(pieces(1, 127))["operands"] == 128 * 76 and dict(pieces(3, 43))["operands"] == 256 * 76
    for S in (2, 31, 64, 128):
        sizes = [q(c, S) for c in range(1, 70)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    for chunk in (1, 7, 100):
        sizes = [q(chunk, S) for S in range(1, 200)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))


class Call:
    """a valid argument list with non-NULL stand-ins for the device pointers (never dereferenced: every case below returns from the
    host-side checks), real host arrays for the level table"""

    def __init__(self):
        from project_nerf_amd import ops
        self.levels = ops.HashLevelTable(16, 14)
        self.a = dict(packed_d=0x1000, packed_c=0x1100, table_f32=0x2000, table_f16=None, levels=16, hash_bound=1.0, grid=0x3000, res=16,
                      grid_bound=1.5, rays_o=0x4000, rays_d=0x5000, n_rays=5, S=8, near=2.0, far=6.0, time=0xb000, bg=None, bg_rows=0,
                      chunk=5, ws=0x10000, rgb=0x6000, depth=0x7000, acc=0x8000, level_arrays=None)

    def run(self, lib, **over):
        a = {**self.a, **over}
        arrays = list(self.levels.host_args()) if a["level_arrays"] is None else a["level_arrays"]
        return lib.nerf_p3_render_rays_fwd(a["packed_d"], a["packed_c"], a["table_f32"], a["table_f16"], a["levels"], *arrays, a["hash_bound"],
                                           a["grid"], a["res"], a["grid_bound"], a["rays_o"], a["rays_d"], a["n_rays"], a["S"], a["near"],
                                           a["far"], a["time"], a["bg"], a["bg_rows"], a["chunk"], a["ws"], a["rgb"], a["depth"], a["acc"],
                                           None)


def test_no_rays_is_a_no_op(lib):
    assert lib.nerf_p3_render_rays_fwd(None, None, None, None, 3, None, None, None, None, None, -1.0, None, 0, -1.0, None, None, 0, 1, 2.0, 6.0,
                                       None, None, 7, 0, None, None, None, None, None) == 0


def _without(call, k):
    arrays = list(call.levels.host_args())
    arrays[k] = None
    return arrays


REFUSALS = [
    ("negative n_rays", dict(n_rays=-1)),
    # counted_render_check's
    ("NULL workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=0x10000 + 128)),
    ("n_samples 1", dict(S=1)),
    ("n_samples 1025", dict(S=1025)),
    ("chunk_rays 0", dict(chunk=0)),
    ("chunk_rays * n_samples = 2^31", dict(chunk=2 ** 21, S=1024)),
    ("bg_rows 2 with n_rays 5", dict(bg=0xa000, bg_rows=2)),
    ("grid_resolution 0", dict(res=0)),
    ("grid_resolution 32769", dict(res=32769)),
    ("NULL grid", dict(grid=None)),
    ("NULL rays_o", dict(rays_o=None)),
    ("NULL rays_d", dict(rays_d=None)),
    ("NULL out_rgb", dict(rgb=None)),
    ("NULL out_depth", dict(depth=None)),
    ("NULL out_acc", dict(acc=None)),
    # the entry's own
    ("both tables", dict(table_f16=0x9000)),
    ("neither table", dict(table_f32=None)),
    ("canon_levels 8", dict(levels=8)),
    ("hash_bound 0", dict(hash_bound=0.0)),
    ("hash_bound negative", dict(hash_bound=-1.0)),
    ("grid_bound 0", dict(grid_bound=0.0)),
    ("grid_bound negative", dict(grid_bound=-1.5)),
    ("NULL packed_deform", dict(packed_d=None)),
    ("NULL packed_canon", dict(packed_c=None)),
    ("NULL time_dev", dict(time=None)),
] + [(f"NULL level array {k}", k) for k in range(5)]


@pytest.mark.parametrize("name,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_arguments_are_refused_on_the_host(lib, name, over):
    lib.nerf_sample_rays(None, None, None, 0, 64, 2.0, 6.0, None, None, None, None)        # a success in between: the message below is this call's
    call = Call()
    if isinstance(over, int):
        over = dict(level_arrays=_without(call, over))
    code = call.run(lib, **over)
    assert code == -22, name
    msg = lib.nerf_last_error()
    assert msg and ENTRY in msg, (name, msg)


def test_the_fp16_table_alone_passes_the_table_check(lib):
    """exactly one table: the fp16 pointer alone gets past that check (and is then refused for the NULL grid, further down)"""
    code = Call().run(lib, table_f32=None, table_f16=0x2000, grid=None)
    assert code == -22 and b"NULL pointer" in lib.nerf_last_error(), lib.nerf_last_error()


def test_ops_refuses_cpu_tensors_and_a_time_vector(lib):
    import torch
    from project_nerf_amd import _lib, ops
    levels = ops.HashLevelTable(16, 14)
    args = (torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8), torch.zeros(levels.entries, 2), levels, 1.0,
            torch.ones(4, 4, 4, dtype=torch.bool), 1.5, torch.zeros(4, 3), torch.zeros(4, 3), 8, 2.0, 6.0)
    with pytest.raises(_lib.NerfHipError):
        ops.p3_render_rays_fwd(*args, torch.zeros(1), None, 4)


def test_abi_version(lib):
    from project_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = int(re.search(r"#define NERF_ABI_VERSION (\d+)", header).group(1))
    assert 14 < declared == _lib.ABI_VERSION == lib.nerf_abi_version()        # the entries are new in version 15
    assert re.search(r"/\* 15: .*nerf_p3_render_", header)


def test_header_cites_the_reference(lib):
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    at = header.index("size_t nerf_p3_render_workspace_bytes")
    comment = header[header.rindex("/* ----", 0, at):at]
    for cite in ("src/renderer.py:240-384", "387-418", "src/core.py:233-281"):
        assert cite in comment, cite
