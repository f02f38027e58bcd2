"""Host-side checks of nerf_instant_render_* (the Instant-NGP evaluation launch chain): the workspace size query against the
layout include/nerf_hip.h documents, and the argument validation, which returns before anything is launched -- no GPU needed."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """the layout of include/nerf_hip.h restated: header, z, slots, pts, dirs, bf16 operand image [roundup(n, 128), 32], rgb, sigma"""
    n = chunk * S
    n_pad = (n + 127) // 128 * 128
    return 256 + up256(n * 4) + up256(n * 4) + up256(n * 12) + up256(n * 12) + up256(n_pad * 32 * 2) + up256(n * 12) + up256(n * 4)


def test_workspace_size_query(lib):
    q = lib.nerf_instant_render_workspace_bytes
    for chunk, S in ((0, 128), (-1, 128), (5, 0), (5, -3), (0, 0)):
        assert q(chunk, S) == 0
    for chunk, S in ((1, 2), (1, 127), (1, 128), (3, 43), (5, 64), (13, 64), (4096, 128), (200000, 128)):
        assert q(chunk, S) == documented_bytes(chunk, S), (chunk, S)
        assert q(chunk, S) % 256 == 0
    # about 112 bytes per sample, not the ~1 KB training layout
    assert 111.9 < q(200000, 128) / (200000 * 128) < 112.1
    assert lib.nerf_imlp_workspace_bytes(200000 * 128) > 8 * q(200000, 128)
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
        self.a = dict(packed=0x1000, table_f32=0x2000, table_f16=None, n_levels=16, hash_bound=1.5, grid=0x3000, res=16, grid_bound=1.5,
                      rays_o=0x4000, rays_d=0x5000, n_rays=5, S=8, near=2.0, far=6.0, bg=None, bg_rows=0, chunk=5, ws=0x10000,
                      rgb=0x6000, depth=0x7000, acc=0x8000)

    def run(self, lib, **over):
        a = {**self.a, **over}
        return lib.nerf_instant_render_rays_fwd(a["packed"], a["table_f32"], a["table_f16"], a["n_levels"], *self.levels.host_args(),
                                                a["hash_bound"], a["grid"], a["res"], a["grid_bound"], a["rays_o"], a["rays_d"], a["n_rays"],
                                                a["S"], a["near"], a["far"], a["bg"], a["bg_rows"], a["chunk"], a["ws"], a["rgb"], a["depth"],
                                                a["acc"], None)


def test_no_rays_is_a_no_op(lib):
    assert lib.nerf_instant_render_rays_fwd(None, None, None, 16, None, None, None, None, None, 1.5, None, 16, 1.5, None, None, 0, 8, 2.0, 6.0,
                                            None, 0, 5, None, None, None, None, None) == 0


@pytest.mark.parametrize("name,over", [
    ("NULL workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=0x10000 + 128)),
    ("n_samples 1", dict(S=1)),
    ("n_samples 1025", dict(S=1025)),
    ("chunk_rays 0", dict(chunk=0)),
    ("chunk_rays * n_samples = 2^31", dict(chunk=2 ** 21, S=1024)),
    ("both tables", dict(table_f16=0x9000)),
    ("neither table", dict(table_f32=None)),
    ("n_levels 8", dict(n_levels=8)),
    ("bg_rows 2 with n_rays 5", dict(bg=0xa000, bg_rows=2)),
    ("grid_resolution 32769", dict(res=32769)),
])
def test_bad_arguments_are_refused_on_the_host(lib, name, over):
    lib.nerf_sample_rays(None, None, None, 0, 64, 2.0, 6.0, None, None, None, None)        # a success in between: the message below is this call's
    code = Call().run(lib, **over)
    assert code < 0, name
    msg = lib.nerf_last_error()
    assert msg and b"nerf_instant_render_rays_fwd" in msg, (name, msg)


def test_ops_refuses_cpu_tensors(lib):
    import torch
    from project_nerf_amd import _lib, ops
    levels = ops.HashLevelTable(16, 14)
    with pytest.raises(_lib.NerfHipError):
        ops.instant_render_rays_fwd(torch.zeros(16, dtype=torch.uint8), torch.zeros(levels.entries, 2), levels, 1.5,
                                    torch.ones(4, 4, 4, dtype=torch.bool), 1.5, torch.zeros(4, 3), torch.zeros(4, 3), 8, 2.0, 6.0, None, 4)
