"""Host-side checks of nerf_p3_grid_update* (the Part 3 occupancy-grid refresh -- MLP deformation, hash-grid canonical field -- as one
density-only launch chain): the workspace size query against the layout include/nerf_hip.h documents, and the argument validation,
which returns before anything is launched -- no GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b"nerf_p3_grid_update"


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


def documented_bytes(slab):
    """the layout of include/nerf_hip.h restated: with rows = roundup(slab, 128), x_c [rows, 3] fp32 and one fp16 operand image
    [rows, 32] of the canonical grid, each piece rounded up to 256 bytes"""
    rows = (slab + 127) // 128 * 128
    up = lambda b: (b + 255) // 256 * 256
    return up(rows * 12) + up(rows * 64)


def test_symbols_are_exported_and_bound(lib):
    from project_nerf_amd import _lib, ops
    for name in ("nerf_p3_grid_update", "nerf_p3_grid_update_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert callable(ops.p3_grid_update) and callable(ops.p3_grid_update_workspace_bytes)
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert "int nerf_p3_grid_update(" in header and "size_t nerf_p3_grid_update_workspace_bytes(int64_t slab_cells);" in header


def test_workspace_size_query(lib):
    from project_nerf_amd import ops
    q = lib.nerf_p3_grid_update_workspace_bytes
    for slab in (0, -1, -128):
        assert q(slab) == 0
    for slab in (1, 128, 129, 256, 384, 2 ** 18):
        assert q(slab) == documented_bytes(slab), slab
        assert q(slab) % 256 == 0
    assert q(2 ** 18) == 76 * 2 ** 18 == 19922944             # 12 + 64 bytes per cell of a slab
    assert q(128) == 128 * 76 == 9728                         # 1536 + 8192: both pieces are multiples of 256 already
    assert q(384) == 384 * 76 == 29184
    assert q(129) == q(256) == 256 * 76
    assert ops.p3_grid_update_workspace_bytes(2 ** 18) == 19922944
    assert q(2 ** 18) < lib.nerf_p4_grid_update_workspace_bytes(2 ** 18)     # no deformation operand image
    sizes = [q(s) for s in range(1, 1201)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes == [documented_bytes(s) for s in range(1, 1201)]


def floats(*values):
    return (ctypes.c_float * len(values))(*values)


class Call:
    """a valid argument list with non-NULL stand-ins for the device pointers (never dereferenced: every case below returns from the
    host-side checks), real host arrays for the level table and the times"""

    def __init__(self):
        from project_nerf_amd import ops
        self.levels = ops.HashLevelTable(16, 14)
        self.a = dict(packed_d=0x1000, packed_c=0x1800, table_f32=0x2000, table_f16=None, canon_levels=16, levels=self.levels.host_args(),
                      hash_bound=1.0, times=floats(0.0, 0.5, 1.0), n_times=3, n_cells=16 ** 3, res=16, grid_bound=1.5, grid=0x3000,
                      binary=0x4000, decay=1.0, threshold=0.01, count=0x5000, slab=2 ** 18, ws=0x10000)

    def run(self, lib, **over):
        a = {**self.a, **over}
        return lib.nerf_p3_grid_update(a["packed_d"], a["packed_c"], a["table_f32"], a["table_f16"], a["canon_levels"], *a["levels"],
                                       a["hash_bound"], a["times"], a["n_times"], a["n_cells"], a["res"], a["grid_bound"], a["grid"],
                                       a["binary"], a["decay"], a["threshold"], a["count"], a["slab"], a["ws"], None)


def without_level_array(k):
    levels = list(Call().levels.host_args())
    levels[k] = None
    return tuple(levels)


@pytest.mark.parametrize("name,over", [
    ("fp32 and fp16 tables", dict(table_f16=0x9000)),
    ("no table", dict(table_f32=None)),
    ("canonical levels 8", dict(canon_levels=8)),
    ("canonical levels 17", dict(canon_levels=17)),
    ("n_times 0", dict(n_times=0)),
    ("n_times -1", dict(n_times=-1)),
    ("n_times 257", dict(times=floats(*([0.5] * 257)), n_times=257)),
    ("NULL times", dict(times=None)),
    ("a NaN time", dict(times=floats(0.0, float("nan"), 1.0))),
    ("an infinite time", dict(times=floats(0.0, 0.5, float("inf")))),
    ("a negative infinite first time", dict(times=floats(float("-inf"), 0.5, 1.0))),
    ("resolution 1", dict(res=1, n_cells=1)),
    ("resolution 32769", dict(res=32769, n_cells=32769 ** 3)),
    ("n_cells is not resolution^3", dict(n_cells=16 ** 3 - 1)),
    ("n_cells 0", dict(n_cells=0)),
    ("slab_cells 0", dict(slab=0)),
    ("slab_cells -128", dict(slab=-128)),
    ("slab_cells 200", dict(slab=200)),
    ("slab_cells * 32 = 2^31", dict(slab=2 ** 26)),
    ("NULL workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=0x10000 + 128)),
    ("hash_bound 0", dict(hash_bound=0.0)),
    ("negative hash_bound", dict(hash_bound=-1.0)),
    ("grid_bound 0", dict(grid_bound=0.0)),
    ("negative grid_bound", dict(grid_bound=-1.5)),
    ("NULL packed_deform", dict(packed_d=None)),
    ("NULL packed_canon", dict(packed_c=None)),
    ("NULL scale array", dict(levels=without_level_array(0))),
    ("NULL resolution array", dict(levels=without_level_array(1))),
    ("NULL size array", dict(levels=without_level_array(2))),
    ("NULL offset array", dict(levels=without_level_array(3))),
    ("NULL dense array", dict(levels=without_level_array(4))),
    ("NULL grid", dict(grid=None)),
    ("NULL binary_grid", dict(binary=None)),
    ("NULL active_count", dict(count=None)),
])
def test_bad_arguments_are_refused_on_the_host(lib, name, over):
    lib.nerf_sample_rays(None, None, None, 0, 64, 2.0, 6.0, None, None, None, None)        # a success in between: the message below is this call's
    code = Call().run(lib, **over)
    assert code == -22, name
    msg = lib.nerf_last_error()
    assert msg and ENTRY in msg, (name, msg)


def test_the_limits_themselves_pass_the_host_checks():
    """256 times, one time and an fp16 table are inside the rules: with a NULL table behind them the call still fails, but on the rule
    that was broken, not on theirs"""
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import _lib
    lib = _lib.load()
    for over in (dict(times=floats(*([0.25] * 256)), n_times=256), dict(times=floats(0.7), n_times=1),
                 dict(table_f32=None, table_f16=0x2000, slab=128), dict(res=2, n_cells=8), dict(slab=2 ** 26 - 128)):
        assert Call().run(lib, **over, grid=None) == -22
        assert b"NULL pointer" in lib.nerf_last_error(), (over, lib.nerf_last_error())


def test_ops_refuses_cpu_tensors(lib):
    import torch
    from project_nerf_amd import _lib, ops
    lv = ops.HashLevelTable(16, 14)
    table = torch.zeros(lv.entries, 2)
    with pytest.raises(_lib.NerfHipError):
        ops.p3_grid_update(torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8), table, lv, 1.0, [0.0, 1.0], 8, 1.5, 0.01,
                           torch.zeros(8, 8, 8))


def test_abi_version(lib):
    from project_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = int(re.search(r"#define NERF_ABI_VERSION (\d+)", header).group(1))
    assert 14 <= declared == _lib.ABI_VERSION == lib.nerf_abi_version()       # the entries are new in version 14
    assert re.search(r"/\* 14: .*nerf_p3_grid_update", header)
