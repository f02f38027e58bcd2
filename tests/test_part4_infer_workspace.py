"""nerf_p4_infer_workspace_bytes -- the evaluation size of the Part 4 workspace (the four fp16 operand images that lead the
layout) -- against the layout include/nerf_hip.h documents, and the Python Workspace's two sizes.  No GPU needed."""
import os

import pytest
import torch

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


def image_bytes(n):
    return (n + 127) // 128 * 128 * 32 * 2               # fp16 operand image [roundup(n, 128), 32]


def test_size_query_is_the_four_leading_images(lib):
    q = lib.nerf_p4_infer_workspace_bytes
    for n in (0, -1, -(2 ** 40)):
        assert q(n) == 0
    for n in (1, 127, 128, 129, 1000, 65536 * 64, 65536 * 128, 2 ** 31 + 5):
        assert q(n) == 4 * image_bytes(n), n
        assert q(n) % 256 == 0
        # the images sit at the head of the training layout, one after the other: an evaluation buffer is a prefix of it
        assert [lib.nerf_p4_workspace_offset(n, k) for k in range(4)] == [k * image_bytes(n) for k in range(4)]
        assert lib.nerf_p4_workspace_offset(n, 4) >= q(n)
        assert q(n) < lib.nerf_p4_workspace_bytes(n)
    n = 65536 * 128
    assert q(n) == 256 * n                               # 256 bytes per sample ...
    assert lib.nerf_p4_workspace_bytes(n) > 10 * q(n)    # ... where the training layout takes ~2.9 KB
    sizes = [q(n) for n in range(1, 700)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


def test_python_workspace_has_two_sizes(lib):
    from project_nerf_amd.part4 import Workspace, forward_chain
    n = 1000
    assert Workspace.bytes(n) == lib.nerf_p4_workspace_bytes(n)
    assert Workspace.bytes(n, train=False) == lib.nerf_p4_infer_workspace_bytes(n) == 4 * image_bytes(n)
    assert Workspace.bytes(0, train=False) == 256        # never an empty tensor
    small = Workspace(n, "cpu", train=False)
    assert small.buf.numel() == 4 * image_bytes(n) and not small.train
    assert [small.nat(k).data_ptr() - small.buf.data_ptr() for k in range(4)] == [k * image_bytes(n) for k in range(4)]
    with pytest.raises(ValueError, match="d features"):
        small.d_feat(0)
    with pytest.raises(ValueError, match="bytes needed"):          # an evaluation-sized buffer cannot back a training workspace
        Workspace(n, "cpu", buf=small.buf)
    Workspace(n, "cpu", buf=small.buf, train=False)
    pts = torch.zeros(n, 3)
    with pytest.raises(ValueError, match="stash"):                 # refused before anything is launched
        forward_chain(None, None, [None] * 4, None, None, 1.5, pts, None, torch.zeros(n), pts, small, True)
