// The slab chain, shared by the three occupancy-grid refresh entries of grid.hip (nerf_instant_grid_update, nerf_p4_grid_update,
// nerf_p3_grid_update): DensityGrid.update (reference src/renderer.py:35-132) for ANY number of cells as one density-only launch
// chain.  All on the caller's stream:
//   clear the count -> per slab of `slab_cells` cells, per pass j = 0 .. n_passes - 1: the entry's field launches, the last of which
//   folds the pass's sigma into grid / binary_grid with nerf_grid_update's running maximum in its epilogue.
// The decay / count rule: the FIRST pass of a slab folds against the decayed history, max(grid * decay, s_0); the others run with
// decay 1, so the cell ends as max(... max(max(g d, s_0), s_1) ..., s_{P-1}) -- the reference's max(g d, max(s_0 .. s_{P-1})), and
// with decay 1 its sequence of updates (a maximum of non-NaN values does not depend on its grouping): the bits of the loop form.
// Only the LAST pass is given the count pointer (the sigma epilogues skip a NULL one): binary_grid and the count are those of the
// finished cell.  The (slab, pass) launches share ONE caller-provided workspace; stream order serialises them.  No lattice tensor,
// no rgb, no view directions, no allocation, no host read: (launches per pass) * n_passes * ceil(n_cells / slab_cells) + 1 enqueues.
// Host code only.  Every refusal begins with `what`, the name of the entry that was called.
#pragma once
#include "common.h"

namespace nerf {

// rows of a slab's pieces: the operand images are padded to a multiple of 128 cells (0: every size query answers 0)
inline size_t slab_rows(int64_t slab_cells) { return slab_cells > 0 ? ((size_t)slab_cells + 127) / 128 * 128 : 0; }

// the lattice source: the cells are the nodes of nerf_grid_lattice(grid_bound, resolution)
inline int slab_lattice_check(const char* what, int resolution, int64_t n_cells, float grid_bound) {
  NERF_REQUIRE(resolution >= 2 && resolution <= 32768, "%s: resolution=%d (2..32768)", what, resolution);
  NERF_REQUIRE(n_cells == (int64_t)resolution * resolution * resolution, "%s: n_cells=%lld is not resolution^3 (%d)", what,
               (long long)n_cells, resolution);
  NERF_REQUIRE(grid_bound > 0.0f, "%s: grid_bound must be positive", what);
  return NERF_OK;
}

// the checks every entry makes of its common arguments (the entry has made its own)
inline int slab_chain_check(const char* what, const float* grid, const uint8_t* binary_grid, const unsigned long long* active_count,
                            int64_t slab_cells, const void* workspace) {
  NERF_REQUIRE(slab_cells > 0 && slab_cells % 128 == 0, "%s: slab_cells=%lld (a positive multiple of 128)", what, (long long)slab_cells);
  NERF_REQUIRE(slab_cells * 32 < ((int64_t)1 << 31), "%s: slab too large (slab_cells * 32 must stay below 2^31)", what);
  NERF_REQUIRE(grid && binary_grid && active_count && workspace, "%s: NULL pointer", what);
  NERF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", what);
  return NERF_OK;
}

// pass(j, c0, n, grid, binary_grid, decay, count) queues the entry's launches of pass j for the n cells from c0 on (grid / binary_grid
// already offset to c0; decay and count by the rule above) and returns their status
template <class Pass>
int slab_chain(const char* what, int64_t n_cells, float* grid, uint8_t* binary_grid, float decay, unsigned long long* active_count,
               int64_t slab_cells, const void* workspace, int n_passes, nerf_stream_t stream, Pass pass) {
  const int ok = slab_chain_check(what, grid, binary_grid, active_count, slab_cells, workspace);
  if (ok != NERF_OK) return ok;
  if (hipMemsetAsync(active_count, 0, sizeof(unsigned long long), as_stream(stream)) != hipSuccess)
    return fail(NERF_ELAUNCH, "%s: memset failed", what);
  for (int64_t c0 = 0; c0 < n_cells; c0 += slab_cells) {
    const int64_t n = n_cells - c0 < slab_cells ? n_cells - c0 : slab_cells;
    for (int j = 0; j < n_passes; ++j) {
      const int rc = pass(j, c0, n, grid + c0, binary_grid + c0, j == 0 ? decay : 1.0f, j == n_passes - 1 ? active_count : nullptr);
      if (rc != NERF_OK) return rc;
    }
  }
  return NERF_OK;
}

}  // namespace nerf
