"""Host-side checks of nerf_p3_nerf_render_* (the evaluation launch chain of Part 3 with the 8x256 canonical field, standard and direct
time conditioning): the workspace size query against the layout include/nerf_hip.h documents, piece by piece, and the argument
validation, which returns before anything is launched -- no GPU needed."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b"nerf_p3_nerf_render_rays_fwd"


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
    """the layout of include/nerf_hip.h restated: z, pts, dirs, x_c, sigma, rgb"""
    n = chunk * S
    return [("z", up256(n * 4)), ("pts", up256(n * 12)), ("dirs", up256(n * 12)), ("x_c", up256(n * 12)), ("sigma", up256(n * 4)),
            ("rgb", up256(n * 12))]


def documented_bytes(chunk, S):
    return sum(b for _, b in pieces(chunk, S))


def header():
    return open(os.path.join(ROOT, "include", "nerf_hip.h")).read()


def test_symbols_are_exported_and_bound(lib):
    """header, library and binding declare the two entries alike"""
    from project_nerf_amd import _lib, ops
    for name in ("nerf_p3_nerf_render_rays_fwd", "nerf_p3_nerf_render_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert callable(ops.p3_nerf_render_rays_fwd) and callable(ops.p3_nerf_render_workspace_bytes)
    h = header()
    assert "size_t nerf_p3_nerf_render_workspace_bytes(int64_t chunk_rays, int n_samples);" in h
    decl = re.search(r"int nerf_p3_nerf_render_rays_fwd\((.*?)\);", h, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["const void* packed_deform", "const void* packed_canon", "const float* rays_o", "const float* rays_d", "int64_t n_rays",
                      "int n_samples", "float near_plane", "float far_plane", "const float* time_dev", "const float* bg", "int64_t bg_rows",
                      "int64_t chunk_rays", "void* workspace", "float* out_rgb", "float* out_depth", "float* out_acc", "nerf_stream_t stream"]
    import ctypes
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int32, "float": ctypes.c_float}
    want = [ctypes.c_void_p if ("*" in p or p.startswith("nerf_stream_t")) else kinds[p.split()[0]] for p in params]
    restype, argtypes = _lib.PROTOTYPES["nerf_p3_nerf_render_rays_fwd"]
    assert list(argtypes) == want and restype is ctypes.c_int32
    assert _lib.PROTOTYPES["nerf_p3_nerf_render_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32])
    source = open(os.path.join(ROOT, "project-nerf_amd", "csrc", "render_p3_nerf.hip")).read()
    assert 'extern "C" int nerf_p3_nerf_render_rays_fwd(' in source and 'extern "C" size_t nerf_p3_nerf_render_workspace_bytes(' in source


def test_workspace_size_query(lib):
    from project_nerf_amd import ops
    q = lib.nerf_p3_nerf_render_workspace_bytes
    for chunk, S in ((0, 128), (-1, 128), (5, 0), (5, -3), (0, 0), (-4, -4)):
        assert q(chunk, S) == 0
    for chunk, S in ((1, 2), (100, 32), (16384, 128), (1, 127), (3, 43), (5, 64), (40, 128)):
        assert q(chunk, S) == documented_bytes(chunk, S), (chunk, S, pieces(chunk, S))
        assert q(chunk, S) % 256 == 0
    assert q(1, 2) == 6 * 256                                     # every piece is smaller than one 256-byte unit
    assert q(100, 32) == 100 * 32 * 56 == 179200                   # 3200 samples: every piece a multiple of 256 already
    assert q(16384, 128) == 2 ** 21 * 56 == 117440512              # the engine's default chunk at 128 samples: 56 bytes per sample
    assert ops.p3_nerf_render_workspace_bytes(16384, 128) == 117440512
    for S in (2, 31, 64, 128):
        sizes = [q(c, S) for c in range(1, 70)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))


class Call:
    """a valid argument list with non-NULL stand-ins for the device pointers (never dereferenced: every case below returns from the
    host-side checks)"""

    def __init__(self):
        self.a = dict(packed_d=0x1000, packed_c=0x1100, rays_o=0x4000, rays_d=0x5000, n_rays=5, S=8, near=2.0, far=6.0, time=0xb000, bg=None,
                      bg_rows=0, chunk=5, ws=0x10000, rgb=0x6000, depth=0x7000, acc=0x8000)

    def run(self, lib, **over):
        a = {**self.a, **over}
        return lib.nerf_p3_nerf_render_rays_fwd(a["packed_d"], a["packed_c"], a["rays_o"], a["rays_d"], a["n_rays"], a["S"], a["near"], a["far"],
                                                a["time"], a["bg"], a["bg_rows"], a["chunk"], a["ws"], a["rgb"], a["depth"], a["acc"], None)


def test_no_rays_is_a_no_op(lib):
    """before any pointer check: every pointer NULL, every size out of range"""
    assert lib.nerf_p3_nerf_render_rays_fwd(None, None, None, None, 0, 1, 2.0, 6.0, None, None, 7, 0, None, None, None, None, None) == 0


REFUSALS = [
    ("negative n_rays", dict(n_rays=-1), b"n_rays"),
    ("n_samples 1", dict(S=1), b"n_samples"),
    ("n_samples 1025", dict(S=1025), b"n_samples"),
    ("chunk_rays 0", dict(chunk=0), b"chunk"),
    ("chunk_rays negative", dict(chunk=-3), b"chunk"),
    ("chunk_rays * n_samples = 2^31", dict(chunk=2 ** 21, S=1024), b"chunk"),
    ("NULL workspace", dict(ws=None), b"NULL"),
    ("misaligned workspace", dict(ws=0x10000 + 128), b"aligned"),
    ("NULL packed_canon", dict(packed_c=None), b"NULL"),
    ("NULL packed_canon, direct time conditioning", dict(packed_c=None, packed_d=None), b"NULL"),
    ("NULL rays_o", dict(rays_o=None), b"NULL"),
    ("NULL rays_d", dict(rays_d=None), b"NULL"),
    ("NULL time_dev", dict(time=None), b"NULL"),
    ("NULL out_rgb", dict(rgb=None), b"NULL"),
    ("NULL out_depth", dict(depth=None), b"NULL"),
    ("NULL out_acc", dict(acc=None), b"NULL"),
    ("bg_rows 2 with n_rays 5", dict(bg=0xa000, bg_rows=2), b"bg_rows"),
    ("bg_rows 0 with a background", dict(bg=0xa000, bg_rows=0), b"bg_rows"),
]


@pytest.mark.parametrize("name,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_arguments_are_refused_on_the_host(lib, name, over, word):
    """NERF_EINVAL with the entry's name and the argument in the message.  Nothing is launched: there is no GPU here, and a launch
    (or the device query in front of it) would come back as NERF_ELAUNCH, not -22."""
    lib.nerf_sample_rays(None, None, None, 0, 64, 2.0, 6.0, None, None, None, None)        # a success in between: the message below is this call's
    code = Call().run(lib, **over)
    assert code == -22, name
    msg = lib.nerf_last_error()
    assert msg and ENTRY in msg and word in msg, (name, msg)


def test_ops_refuses_cpu_tensors_and_a_time_vector(lib):
    import torch
    from project_nerf_amd import _lib, ops
    packed = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(_lib.NerfHipError):
        ops.p3_nerf_render_rays_fwd(packed, packed, torch.zeros(4, 3), torch.zeros(4, 3), 8, 2.0, 6.0, torch.zeros(1), None, 4)
    with pytest.raises(_lib.NerfHipError):
        ops.p3_nerf_render_rays_fwd(None, packed, torch.zeros(4, 3), torch.zeros(4, 3), 8, 2.0, 6.0, torch.zeros(1), None, 4)


def test_abi_version(lib):
    from project_nerf_amd import _lib
    h = header()
    declared = int(re.search(r"#define NERF_ABI_VERSION (\d+)", h).group(1))
    assert 16 <= declared == _lib.ABI_VERSION == lib.nerf_abi_version()       # the entries are new in version 16
    assert re.search(r"/\* 16: .*nerf_p3_nerf_render_", h)


def test_header_cites_the_reference(lib):
    h = header()
    at = h.index("size_t nerf_p3_nerf_render_workspace_bytes")
    comment = h[h.rindex("/* ----", 0, at):at]
    for cite in ("src/renderer.py:387-418", "src/core.py:108-146"):
        assert cite in comment, cite
    decl = h[at:h.index(";", h.index("int nerf_p3_nerf_render_rays_fwd(", at))]
    assert "NULL: direct time conditioning" in decl and "direct time conditioning" in comment
