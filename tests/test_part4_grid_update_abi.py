"""Host-side checks of nerf_p4_grid_update* (the Part 4 occupancy-grid refresh as one density-only launch chain): the workspace size
query against the layout include/nerf_hip.h documents, and the argument validation, which returns before anything is launched --
no GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b"nerf_p4_grid_update"


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
    """the layout of include/nerf_hip.h restated: with rows = roundup(slab, 128), one fp16 operand image [rows, 32] of a deformation
    grid, x_c [rows, 3] fp32 and one fp16 operand image [rows, 32] of the canonical grid, each piece rounded up to 256 bytes"""
    rows = (slab + 127) // 128 * 128
    up = lambda b: (b + 255) // 256 * 256
    return up(rows * 64) + up(rows * 12) + up(rows * 64)


def test_workspace_size_query(lib):
    q = lib.nerf_p4_grid_update_workspace_bytes
    for slab in (0, -1, -128):
        assert q(slab) == 0
    for slab in (1, 128, 129, 256, 384, 2 ** 18):
        assert q(slab) == documented_bytes(slab), slab
        assert q(slab) % 256 == 0
    assert q(2 ** 18) == 140 * 2 ** 18 == 36700160            # 64 + 12 + 64 bytes per cell of a slab
    assert lib.nerf_p4_infer_workspace_bytes(2 ** 18) == 256 * 2 ** 18      # the loop form's four operand images per batch
    sizes = [q(s) for s in range(1, 1201)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes == [documented_bytes(s) for s in range(1, 1201)]


class Call:
    """a valid argument list with non-NULL stand-ins for the device pointers (never dereferenced: every case below returns from the
    host-side checks), real host arrays for the two level tables and the table-pointer array"""

    def __init__(self):
        from project_nerf_amd import ops
        self.levels_d, self.levels_c = ops.HashLevelTable(12, 12), ops.HashLevelTable(16, 14)
        self.tables = (ctypes.c_void_p * 4)(0x2000, 0x2100, 0x2200, 0x2300)
        self.a = dict(packed=0x1000, params=0x1800, tables_f32=self.tables, tables_f16=None, deform_levels=12, canon_levels=16, hash_bound=1.5,
                      n_cells=16 ** 3, res=16, grid_bound=1.5, grid=0x3000, binary=0x4000, decay=0.95, threshold=0.01, count=0x5000,
                      slab=2 ** 18, ws=0x10000)

    def run(self, lib, **over):
        a = {**self.a, **over}
        return lib.nerf_p4_grid_update(a["packed"], a["params"], a["tables_f32"], a["tables_f16"], a["deform_levels"],
                                       *self.levels_d.host_args(), a["canon_levels"], *self.levels_c.host_args(), a["hash_bound"],
                                       a["n_cells"], a["res"], a["grid_bound"], a["grid"], a["binary"], a["decay"], a["threshold"], a["count"],
                                       a["slab"], a["ws"], None)


HOLE = (ctypes.c_void_p * 4)(0x2000, 0x2100, None, 0x2300)
OTHER = (ctypes.c_void_p * 4)(0x9000, 0x9100, 0x9200, 0x9300)


@pytest.mark.parametrize("name,over", [
    ("fp32 and fp16 tables", dict(tables_f16=OTHER)),
    ("no tables", dict(tables_f32=None)),
    ("one table missing", dict(tables_f32=HOLE)),
    ("one fp16 table missing", dict(tables_f32=None, tables_f16=HOLE)),
    ("deformation levels 14", dict(deform_levels=14)),
    ("canonical levels 8", dict(canon_levels=8)),
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
    ("negative grid_bound", dict(grid_bound=-1.5)),
    ("NULL packed", dict(packed=None)),
    ("NULL params", dict(params=None)),
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


def test_ops_refuses_cpu_tensors(lib):
    import torch
    from project_nerf_amd import _lib, ops
    ld, lc = ops.HashLevelTable(12, 12), ops.HashLevelTable(16, 14)
    tables = [torch.zeros(ld.entries, 2)] * 3 + [torch.zeros(lc.entries, 2)]
    with pytest.raises(_lib.NerfHipError):
        ops.p4_grid_update(torch.zeros(16, dtype=torch.uint8), torch.zeros(30145), tables, ld, lc, 1.5, 8, 1.5, 0.01, torch.zeros(8, 8, 8), 0.95)


def test_abi_version(lib):
    from project_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = int(re.search(r"#define NERF_ABI_VERSION (\d+)", header).group(1))
    assert 13 <= declared == _lib.ABI_VERSION == lib.nerf_abi_version()       # the entries are new in version 13
