"""Host-side checks of nerf_render_rays_grid_* (the vanilla field's evaluation through an occupancy grid as one launch chain): the
workspace size query against the layout include/nerf_hip.h documents, the argument validation and the option refusals, which
return before anything is launched, and the agreement of header, library and ctypes table -- no GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


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


def documented_bytes(chunk, S):
    """the layout of include/nerf_hip.h restated: header (the count word), z, slots, pts, dirs, rgb, sigma"""
    n = chunk * S
    return 256 + up256(n * 4) + up256(n * 4) + up256(n * 12) + up256(n * 12) + up256(n * 12) + up256(n * 4)


def test_workspace_size_query(lib):
    q = lib.nerf_render_rays_grid_workspace_bytes
    for chunk, S in ((0, 128), (-1, 128), (5, 0), (5, -3), (0, 0)):
        assert q(chunk, S) == 0
    for chunk, S in ((1, 2), (1, 127), (1, 128), (3, 43), (5, 64), (13, 64), (600, 128), (4096, 128), (200000, 128)):
        assert q(chunk, S) == documented_bytes(chunk, S), (chunk, S)
        assert q(chunk, S) % 256 == 0
    # 48 bytes per sample
    assert 47.99 < q(200000, 128) / (200000 * 128) < 48.01
    for S in (2, 31, 64, 128):
        sizes = [q(c, S) for c in range(1, 70)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))


VALID = dict(packed=0x1000, grid=0x3000, res=16, grid_bound=1.5, rays_o=0x4000, rays_d=0x5000, n_rays=5, S=8, near=2.0, far=6.0, bg=None,
             bg_rows=0, chunk=5, ws=0x10000, rgb=0x6000, depth=0x7000, acc=0x8000)


def run(lib, **over):
    """a valid argument list with non-NULL stand-ins for the device pointers (never dereferenced: every case here returns from the
    host-side checks)"""
    a = {**VALID, **over}
    return lib.nerf_render_rays_grid_fwd(a["packed"], a["grid"], a["res"], a["grid_bound"], a["rays_o"], a["rays_d"], a["n_rays"], a["S"],
                                         a["near"], a["far"], a["bg"], a["bg_rows"], a["chunk"], a["ws"], a["rgb"], a["depth"], a["acc"], None)


def test_no_rays_is_a_no_op(lib):
    assert lib.nerf_render_rays_grid_fwd(None, None, 16, 1.5, None, None, 0, 8, 2.0, 6.0, None, 0, 5, None, None, None, None, None) == 0


@pytest.mark.parametrize("name,over", [
    ("n_rays -1", dict(n_rays=-1)),
    ("NULL workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=0x10000 + 128)),
    ("NULL packed", dict(packed=None)),
    ("NULL grid", dict(grid=None)),
    ("NULL out_rgb", dict(rgb=None)),
    ("n_samples 1", dict(S=1)),
    ("n_samples 1025", dict(S=1025)),
    ("chunk_rays 0", dict(chunk=0)),
    ("chunk_rays * n_samples = 2^31", dict(chunk=2 ** 21, S=1024)),
    ("bg_rows 2 with n_rays 5", dict(bg=0xa000, bg_rows=2)),
    ("grid_resolution 0", dict(res=0)),
    ("grid_resolution 32769", dict(res=32769)),
    ("grid_bound 0", dict(grid_bound=0.0)),
])
def test_bad_arguments_are_refused_on_the_host(lib, name, over):
    lib.nerf_sample_rays(None, None, None, 0, 64, 2.0, 6.0, None, None, None, None)        # a success in between: the message below is this call's
    code = run(lib, **over)
    assert code == EINVAL, name
    msg = lib.nerf_last_error()
    assert msg and b"nerf_render_rays_grid_fwd" in msg, (name, msg)


@pytest.mark.parametrize("option,value,default", [("chain_legacy", 1, 0), ("infer_shape32", 1, 0), ("infer64", 0, 1)])
def test_options_of_another_kernel_family_are_refused_by_name(lib, option, value, default):
    """only the default inference kernel has a counted form: under an option that makes nerf_mlp_fwd launch another kernel the
    entry refuses (its results equal nerf_mlp_fwd's bit for bit, or it does not run) and names the option"""
    assert lib.nerf_set_option(option.encode(), value) == 0
    try:
        assert run(lib) == EINVAL
        msg = lib.nerf_last_error()
        assert b"nerf_render_rays_grid_fwd" in msg and option.encode() in msg, msg
    finally:
        assert lib.nerf_set_option(option.encode(), default) == 0


def test_header_library_and_ctypes_table_agree(lib):
    from project_nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("nerf_render_rays_grid_workspace_bytes", 2), ("nerf_render_rays_grid_fwd", 18)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(handle, name)
    declared = int(re.search(r"#define NERF_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "nerf_hip.h")).read()).group(1))
    assert 10 <= declared == _lib.ABI_VERSION == lib.nerf_abi_version()       # the entries are new in version 10


def test_ops_refuses_cpu_tensors(lib):
    import torch
    from project_nerf_amd import _lib, ops
    with pytest.raises(_lib.NerfHipError):
        ops.render_rays_grid_fwd(torch.zeros(16, dtype=torch.uint8), torch.ones(4, 4, 4, dtype=torch.bool), 1.5, torch.zeros(4, 3),
                                 torch.zeros(4, 3), 8, 2.0, 6.0, None, 4)
