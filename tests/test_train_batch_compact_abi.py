"""Host-side checks of nerf_train_batch_compact / nerf_train_batch_compact_chain (the data side of a training step through the
occupancy grid in one launch): every refusal returns before anything is launched and names the argument, a batch of zero rays
is a no-op, header, library and ctypes table agree -- and the refresh schedule of the grid-training loop
(flat_engine.grid_refresh_due) at its edges.  No GPU needed."""
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


# non-NULL stand-ins for the device pointers, 16-byte aligned (never dereferenced: every case below returns from the host-side checks)
VALID = dict(images=0x1000, poses=0x2000, n_images=3, H=8, W=8, focal=10.0, scene_scale=1.0, bg=0x3000, seed=1, counter=5, first_ray=0,
             batch=7, S=8, near=2.0, far=6.0, grid=0x4000, res=8, bound=1.5, rays_o=0x5000, rays_d=0x6000, rgba=None, target=0x7000,
             z=0x8000, slots=0x9000, pts=0xa000, dirs=0xb000, count=0xc000, turn=0, host=0xd000, seq=1)
ORDER = ("images", "poses", "n_images", "H", "W", "focal", "scene_scale", "bg", "seed", "counter", "first_ray", "batch", "S", "near", "far",
         "grid", "res", "bound", "rays_o", "rays_d", "rgba", "target", "z", "slots", "pts", "dirs", "count")


def run(lib, form, **over):
    a = {**VALID, **over}
    args = [a[k] for k in ORDER]
    if form == "plain":
        return lib.nerf_train_batch_compact(*args, None)
    return lib.nerf_train_batch_compact_chain(*args, a["turn"], a["host"], a["seq"], None)


REFUSALS = [
    ("batch -1", dict(batch=-1), b"batch"),
    ("n_samples 1", dict(S=1), b"n_samples"),
    ("batch * n_samples = 2^31", dict(batch=2 ** 21, S=1024), b"batch * n_samples"),
    ("counter 2^24", dict(counter=2 ** 24), b"counter"),
    ("first_ray -1", dict(first_ray=-1), b"first_ray"),
    ("resolution 0", dict(res=0), b"resolution"),
    ("resolution 32769", dict(res=32769), b"resolution"),
    ("bound 0", dict(bound=0.0), b"bound"),
    ("bound negative", dict(bound=-1.5), b"bound"),
    ("n_images 0", dict(n_images=0), b"n_images"),
    ("H 0", dict(H=0), b"H="),
    ("W 0", dict(W=0), b"W="),
    ("bg without target", dict(target=None, rgba=0xe000), b"target and bg"),
    ("target without bg", dict(bg=None), b"target and bg"),
    ("NULL images", dict(images=None), b"images"),
    ("NULL poses", dict(poses=None), b"poses"),
    ("NULL binary_grid", dict(grid=None), b"binary_grid"),
    ("NULL rays_o", dict(rays_o=None), b"rays_o"),
    ("NULL rays_d", dict(rays_d=None), b"rays_d"),
    ("NULL rgba and target", dict(target=None, bg=None), b"rgba and target"),
    ("NULL z_out", dict(z=None), b"z_out"),
    ("NULL slot_of_sample", dict(slots=None), b"slot_of_sample"),
    ("NULL pts_compact", dict(pts=None), b"pts_compact"),
    ("NULL dirs_compact", dict(dirs=None), b"dirs_compact"),
]


@pytest.mark.parametrize("form", ["plain", "chain"])
@pytest.mark.parametrize("name,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_arguments_are_refused_on_the_host(lib, form, name, over, word):
    lib.nerf_sample_rays(None, None, None, 0, 64, 2.0, 6.0, None, None, None, None)        # a success in between: the message below is this call's
    assert run(lib, form, **over) == EINVAL, name
    msg = lib.nerf_last_error()
    entry = b"nerf_train_batch_compact_chain" if form == "chain" else b"nerf_train_batch_compact"
    assert msg and entry in msg and word in msg, (name, msg)


def test_count_word_and_turn(lib):
    assert run(lib, "plain", count=None) == EINVAL and b"active_count" in lib.nerf_last_error()
    assert run(lib, "chain", count=None) == EINVAL and b"chain_state" in lib.nerf_last_error()
    for turn in (-1, 2):
        assert run(lib, "chain", turn=turn) == EINVAL and b"turn" in lib.nerf_last_error()


def test_no_rays_is_a_no_op_before_any_pointer_check(lib):
    none = [None if k in ("images", "poses", "bg", "grid", "rays_o", "rays_d", "rgba", "target", "z", "slots", "pts", "dirs", "count")
            else VALID[k] for k in ORDER]
    none[ORDER.index("batch")] = 0
    assert lib.nerf_train_batch_compact(*none, None) == 0
    assert lib.nerf_train_batch_compact_chain(*none, 0, None, 1, None) == 0


def test_header_library_and_ctypes_table_agree(lib):
    from project_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("nerf_train_batch_compact", 28), ("nerf_train_batch_compact_chain", 31)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(handle, name)
    declared = int(re.search(r"#define NERF_ABI_VERSION (\d+)", header).group(1))
    assert 11 <= declared == _lib.ABI_VERSION == lib.nerf_abi_version()       # the entries are new in version 11


def test_refresh_schedule_at_its_edges():
    """first refresh after step `warm`, then every 32 / 128 / 512 steps below 10 % / 50 % / `stop` of the run"""
    from project_nerf_amd.flat_engine import grid_refresh_due as due
    iters, warm, stop = 10240, 256, 0.9
    assert not due(warm - 1, iters, warm, stop) and due(warm, iters, warm, stop)
    assert not any(due(s, iters, warm, stop) for s in range(1, warm))               # dense steps: nothing to refresh with
    assert due(288, iters, warm, stop) and not due(289, iters, warm, stop)          # every 32 ...
    assert due(992, iters, warm, stop)                                              # ... up to the last multiple below 10 %
    assert not due(1056, iters, warm, stop) and due(1024, iters, warm, stop)        # from 10 % (1024): every 128
    assert due(1152, iters, warm, stop) and due(4992, iters, warm, stop)
    assert due(5120, iters, warm, stop) and not due(5248, iters, warm, stop)        # from 50 % (5120): every 512
    assert due(8704, iters, warm, stop)                                             # the last one below stop = 9216
    assert not due(9216, iters, warm, stop) and not due(9728, iters, warm, stop)    # none from `stop` on
    assert [s for s in range(1, iters + 1) if due(s, iters, warm, stop)][:3] == [256, 288, 320]
    # a short run: the first refresh alone (warm is no multiple of an interval), and it comes even past `stop`
    assert [s for s in range(1, 13) if due(s, 12, 4, 0.9)] == [4]
    assert [s for s in range(1, 13) if due(s, 12, 11, 0.9)] == [11]
    assert [s for s in range(1, 401) if due(s, 400, 0, 0.9)] == [1, 32, 128]            # (40 and 200 are the 10 % and 50 % marks)


def test_ops_refuses_cpu_tensors(lib):
    import torch
    from project_nerf_amd import _lib, ops
    with pytest.raises(_lib.NerfHipError):
        ops.train_batch_compact(torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4), 5.0, 4, 8, 2.0, 6.0, 0, 1, torch.ones(4, 4, 4, dtype=torch.bool),
                                1.5, bg=torch.ones(3))
