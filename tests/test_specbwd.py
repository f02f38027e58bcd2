"""Host-side bookkeeping of the speculative hash backward (project-nerf_amd/specbwd.py::SpeculativeScatter) without a GPU: the
status blocks are plain int32 tensors the test fills the way the call's last launch does ([3] overflowed records, [4] lost,
[6] scaled, [7] published, written last), the workspaces plain CPU tensors (only their addresses matter)."""
import warnings

import pytest
import torch

import project_nerf_amd  # noqa: F401
from project_nerf_amd import ops
from project_nerf_amd.specbwd import SpeculativeScatter


def scatter(enabled=True):
    s = SpeculativeScatter(enabled)
    s._status = torch.zeros(2, 8, dtype=torch.int32)          # instead of the host-mapped pinned blocks
    return s


def publish(block, overflow=0, lost=0, scaled=0):
    """what hash_bin_overflow_kernel's last workgroup writes"""
    block[:7] = torch.tensor([1, 2, 3, overflow, lost, 2, scaled], dtype=torch.int32)
    block[7] = 1


WS = torch.zeros(64, dtype=torch.uint8)
OTHER = torch.zeros(64, dtype=torch.uint8)
GRID = (1234, 0)


def test_window_edges_and_gates():
    assert not ops.deterministic()
    s = scatter()
    assert not s.ok(WS.data_ptr(), GRID, 1000)                # no estimates yet
    s.counted(WS, GRID, 1000)
    # 0.5 n_last <= n <= 1.1 n_last, both edges included
    assert s.ok(WS.data_ptr(), GRID, 500) and not s.ok(WS.data_ptr(), GRID, 499)
    assert s.ok(WS.data_ptr(), GRID, 1100) and not s.ok(WS.data_ptr(), GRID, 1101)
    assert s.ok(WS.data_ptr(), GRID, 1000)
    # another workspace, another occupancy grid (its address or its version)
    assert not s.ok(OTHER.data_ptr(), GRID, 1000)
    assert not s.ok(WS.data_ptr(), (1235, 0), 1000) and not s.ok(WS.data_ptr(), (1234, 1), 1000)
    # the window follows the LAST call
    s.counted(WS, GRID, 2000)
    assert not s.ok(WS.data_ptr(), GRID, 999) and s.ok(WS.data_ptr(), GRID, 1000) and s.ok(WS.data_ptr(), GRID, 2200)
    s.invalidate()
    assert not s.ok(WS.data_ptr(), GRID, 2000)
    assert not scatter(False).ok(WS.data_ptr(), GRID, 1000)
    off = scatter(False)
    off.counted(WS, GRID, 1000)
    assert not off.ok(WS.data_ptr(), GRID, 1000)


def test_counted_and_invalidate_reset_the_clean_header():
    s = scatter()
    s.counted(WS, GRID, 1000)
    assert s._clean is None                                   # a counted call leaves a used header: begin() has to clear it
    block = s.status_block()
    s.issued(WS, GRID, 1000, block)
    assert s._clean == WS.data_ptr() and s.calls == 1 and s.last_status is block
    assert s._from == (WS.data_ptr(), GRID, 1000)
    s.counted(WS, GRID, 900)
    assert s._clean is None and s._from == (WS.data_ptr(), GRID, 900)
    s.issued(WS, GRID, 900, block)
    s.invalidate()
    assert s._clean is None and s._from is None and s.calls == 2


def test_blocks_alternate_and_are_read_before_reuse():
    s = scatter()
    s.counted(WS, GRID, 1000)
    a = s.status_block()
    assert int(a[7]) == 0
    s.issued(WS, GRID, 1000, a)
    b = s.status_block()
    assert a.data_ptr() != b.data_ptr()
    s.issued(WS, GRID, 1000, b)
    assert set(s._checks) == {0, 1}
    publish(a, overflow=7, scaled=1)
    publish(b, overflow=5)
    a2 = s.status_block()                                     # the block of two calls ago: read, then handed out cleared
    assert a2.data_ptr() == a.data_ptr() and int(a2[7]) == 0
    assert s.overflow_max == 7 and s.scaled_calls == 1 and s.lost_calls == 0 and s.enabled
    assert len(s._checks) == 1 and s._checks[s._turn ^ 1] is b
    s.issued(WS, GRID, 1000, a2)
    b2 = s.status_block()
    assert b2.data_ptr() == b.data_ptr() and s.overflow_max == 7 and s.scaled_calls == 1
    # a status word [3] above 2^31 reads as the unsigned count it is
    s.issued(WS, GRID, 1000, b2)
    publish(a2, overflow=-(1 << 31))
    assert s.ok(WS.data_ptr(), GRID, 1000) and s.overflow_max == 1 << 31


def test_unpublished_block_is_not_read_by_ok():
    s = scatter()
    s.counted(WS, GRID, 1000)
    a = s.status_block()
    s.issued(WS, GRID, 1000, a)
    a[:7] = torch.tensor([1, 2, 3, 9, 1, 2, 1], dtype=torch.int32)          # words of a call still in flight; [7] == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert s.ok(WS.data_ptr(), GRID, 1000)
    assert s.enabled and s.lost_calls == 0 and s.overflow_max == 0 and s.scaled_calls == 0
    assert len(s._checks) == 1 and s._checks[s._turn] is a


def test_lost_block_warns_once_and_disables_for_good():
    s = scatter()
    s.counted(WS, GRID, 1000)
    a = s.status_block()
    s.issued(WS, GRID, 1000, a)
    b = s.status_block()
    s.issued(WS, GRID, 1000, b)
    publish(a, overflow=(1 << 20) + 8988, lost=1)
    publish(b, overflow=3)
    with pytest.warns(UserWarning, match="records were lost") as caught:
        assert not s.ok(WS.data_ptr(), GRID, 1000)
    assert len(caught) == 1
    assert not s.enabled and s.lost_calls == 1 and s.overflow_max == (1 << 20) + 8988 and not s._checks
    with warnings.catch_warnings():
        warnings.simplefilter("error")                        # nothing left to warn about, and nothing re-enables the form
        s.counted(WS, GRID, 1000)
        assert not s.ok(WS.data_ptr(), GRID, 1000)
        s.invalidate()
        s.counted(WS, GRID, 1000)
        assert not s.ok(WS.data_ptr(), GRID, 1000)
    assert s.lost_calls == 1
