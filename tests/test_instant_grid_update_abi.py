"""Host-side checks of nerf_instant_grid_update* (the Instant-NGP occupancy-grid refresh as one density-only launch chain): the
workspace size query against the layout include/nerf_hip.h documents, and the argument validation, which returns before anything
is launched -- no GPU needed."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b"nerf_instant_grid_update"


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
    """the layout of include/nerf_hip.h restated: one slab's bf16 operand image [roundup(slab, 128), 32], rounded up to 256 bytes"""
    rows = (slab + 127) // 128 * 128
    return (rows * 64 + 255) // 256 * 256


def test_workspace_size_query(lib):
    q = lib.nerf_instant_grid_update_workspace_bytes
    for slab in (0, -1):
        assert q(slab) == 0
    for slab in (128, 256, 2 ** 18):
        assert q(slab) == documented_bytes(slab), slab
        assert q(slab) % 256 == 0
    assert q(2 ** 18) == 64 * 2 ** 18                      # 64 B per cell of a slab, not the ~1 KB per point of the training layout
    assert lib.nerf_imlp_workspace_bytes(2 ** 18) > 8 * q(2 ** 18)
    sizes = [q(s) for s in range(1, 1200)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


class Call:
    """a valid lattice-source argument list with non-NULL stand-ins for the device pointers (never dereferenced: every case below
    returns from the host-side checks), real host arrays for the level table"""

    def __init__(self):
        from project_nerf_amd import ops
        self.levels = ops.HashLevelTable(16, 14)
        self.a = dict(packed=0x1000, table_f32=0x2000, table_f16=None, n_levels=16, hash_bound=1.5, pts=None, n_cells=16 ** 3, res=16,
                      grid_bound=1.5, grid=0x3000, binary=0x4000, decay=1.0, dynamic=0, threshold=0.01, count=0x5000, slab=2 ** 18,
                      ws=0x10000)

    def run(self, lib, **over):
        a = {**self.a, **over}
        return lib.nerf_instant_grid_update(a["packed"], a["table_f32"], a["table_f16"], a["n_levels"], *self.levels.host_args(),
                                            a["hash_bound"], a["pts"], a["n_cells"], a["res"], a["grid_bound"], a["grid"], a["binary"],
                                            a["decay"], a["dynamic"], a["threshold"], a["count"], a["slab"], a["ws"], None)


@pytest.mark.parametrize("name,over", [
    ("both tables", dict(table_f16=0x9000)),
    ("neither table", dict(table_f32=None)),
    ("n_levels 8", dict(n_levels=8)),
    ("NULL workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=0x10000 + 128)),
    ("slab_cells 0", dict(slab=0)),
    ("slab_cells -128", dict(slab=-128)),
    ("slab_cells 200", dict(slab=200)),
    ("resolution 1", dict(res=1, n_cells=1)),
    ("resolution 32769", dict(res=32769, n_cells=32769 ** 3)),
    ("n_cells is not resolution^3", dict(n_cells=16 ** 3 - 1)),
    ("n_cells 0 with the lattice source", dict(n_cells=0)),
    ("negative n_cells with a point buffer", dict(pts=0xa000, res=0, n_cells=-1)),
    ("point buffer with a resolution", dict(pts=0xa000, res=16, n_cells=16 ** 3)),
    ("NULL grid", dict(grid=None)),
    ("NULL binary_grid", dict(binary=None)),
    ("NULL active_count", dict(count=None)),
    ("NULL packed", dict(packed=None)),
    ("slab_cells * 32 = 2^31", dict(slab=2 ** 26)),
    ("slab_cells * 32 = 2^31 with a point buffer", dict(pts=0xa000, res=0, n_cells=5, slab=2 ** 26)),
])
def test_bad_arguments_are_refused_on_the_host(lib, name, over):
    lib.nerf_sample_rays(None, None, None, 0, 64, 2.0, 6.0, None, None, None, None)        # a success in between: the message below is this call's
    code = Call().run(lib, **over)
    assert code < 0, name
    msg = lib.nerf_last_error()
    assert msg and ENTRY in msg, (name, msg)


def test_no_points_is_a_no_op(lib):
    assert Call().run(lib, pts=0xa000, res=0, n_cells=0) == 0
    # nothing else is looked at
    assert lib.nerf_instant_grid_update(None, None, None, 16, None, None, None, None, None, 1.5, 0xa000, 0, 0, 1.5, None, None, 1.0, 0, 0.01,
                                        None, 2 ** 18, None, None) == 0


def test_ops_refuses_cpu_tensors(lib):
    import torch
    from project_nerf_amd import _lib, ops
    levels = ops.HashLevelTable(16, 14)
    with pytest.raises(_lib.NerfHipError):
        ops.instant_grid_update(torch.zeros(16, dtype=torch.uint8), torch.zeros(levels.entries, 2), levels, 1.5, 8, 1.5, 0.01)
    with pytest.raises(_lib.NerfHipError):
        ops.instant_grid_update(torch.zeros(16, dtype=torch.uint8), torch.zeros(levels.entries, 2), levels, 1.5, torch.zeros(5, 3), 1.5, 0.01)


def test_abi_version(lib):
    from project_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = int(re.search(r"#define NERF_ABI_VERSION (\d+)", header).group(1))
    assert 12 <= declared == _lib.ABI_VERSION == lib.nerf_abi_version()
