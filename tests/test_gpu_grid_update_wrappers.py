"""ops.instant_grid_update, ops.p4_grid_update and ops.p3_grid_update share one argument helper (ops._grid_update_args): each wrapper
refuses a resolution below 2, a ``prev`` that cannot be updated in place, a workspace that is too small and a slab the entry does
not take -- all before any launch -- and one valid call on the smallest grid the entries accept (2^3 cells, one partial tile)
returns tensors of the documented shapes and types with a count that agrees with the binary grid.  Seeded tables and networks, no
trained field; what the chains compute is pinned by test_gpu_{instant,part4,part3}_grid_update.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND, THRESHOLD, SLAB = 1.5, 0.01, 128


def seeded(n, seed, scale=0.1):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


@pytest.fixture(scope="module")
def wrappers():
    """name -> (call(resolution, prev, **kw), the entry's name, whether ``prev`` may be left out)"""
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import ops, part3, part4
    lv_c, lv_d = ops.HashLevelTable(16, 14), ops.HashLevelTable(12, 12)
    table = seeded(2 * lv_c.entries, 1).view(-1, 2)
    tables = [seeded(2 * lv_d.entries, 2 + k).view(-1, 2) for k in range(3)] + [table]
    imlp = ops.imlp_pack(seeded(ops.IMLP_PARAM_COUNT, 5))
    net = seeded(part4.N_PARAMS, 6)
    packed_c, packed_d = part4.pack(net), part3.deform_pack(seeded(part3.N_DEFORM, 7))
    return {
        "instant": (lambda res, prev, **kw: ops.instant_grid_update(imlp, table, lv_c, BOUND, res, BOUND, THRESHOLD, prev, **kw),
                    "nerf_instant_grid_update", True),
        "part4": (lambda res, prev, **kw: ops.p4_grid_update(packed_c, net, tables, lv_d, lv_c, BOUND, res, BOUND, THRESHOLD, prev, 0.95, **kw),
                  "nerf_p4_grid_update", False),
        "part3": (lambda res, prev, **kw: ops.p3_grid_update(packed_d, packed_c, table, lv_c, BOUND, [0.0, 1.0], res, BOUND, THRESHOLD, prev,
                                                             **kw), "nerf_p3_grid_update", False),
    }


@pytest.mark.parametrize("name", ["instant", "part4", "part3"])
def test_wrapper_refusals_and_smallest_grid(wrappers, name):
    from project_nerf_amd import _lib
    call, entry, prev_optional = wrappers[name]
    zeros = lambda *shape: torch.zeros(*shape, device="cuda")
    with pytest.raises(ValueError, match="resolution"):
        call(1, zeros(1), slab_cells=SLAB)
    with pytest.raises(ValueError, match="in place"):
        call(8, zeros(8, 8, 4), slab_cells=SLAB)
    with pytest.raises(ValueError, match="in place"):
        call(8, zeros(8, 8, 16)[:, :, ::2], slab_cells=SLAB)                 # one value per cell, but not contiguous
    with pytest.raises(ValueError, match="workspace"):
        call(8, zeros(8, 8, 8), slab_cells=SLAB, workspace=torch.empty(256, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.NerfHipError, match=entry):
        call(8, zeros(8, 8, 8), slab_cells=200)

    prev = torch.full((2, 2, 2), 0.5, device="cuda")
    for given in ([prev, None] if prev_optional else [prev]):
        grid, binary, count = call(2, given, slab_cells=SLAB)
        assert (grid is prev) == (given is not None)
        assert grid.shape == binary.shape == (2, 2, 2) and count.shape == (1,)
        assert (grid.dtype, binary.dtype, count.dtype) == (torch.float32, torch.bool, torch.int64)
        assert grid.is_cuda and binary.is_cuda and count.is_cuda
        assert int(count) == int(binary.sum())
        assert torch.equal(binary, grid > THRESHOLD)                         # the binary grid is the finished cell's
