// The occupancy grid's lattice (reference src/renderer.py:49-54), shared by grid.hip (nerf_grid_lattice writes the nodes out) and
// hashgrid.hip (the lattice-sourced gather forms them from the cell index): ONE function for a node's coordinate, so that both
// see the same bits.
#pragma once
#include <stdint.h>

namespace nerf {

// spacing of torch.linspace(-b, b, res), formed on the host once per call
inline float lattice_step(float bound, int res) { return (bound - (-bound)) / (float)(res - 1); }

// node i of torch.linspace(-b, b, res): walk up from the start in the lower half, down from the
// end in the upper half (one rounding each)
__device__ __forceinline__ float lattice_node(int i, int res, float bound, float step) {
  return i < res / 2 ? __builtin_fmaf(step, (float)i, -bound) : __builtin_fmaf(-step, (float)(res - 1 - i), bound);
}

// cell c of the 'ij' meshgrid (x slowest, renderer.py:53-54) -> (ix, iy, iz); c < res^3, res <= 32768
__device__ __forceinline__ void lattice_cell(int64_t c, int res, int& ix, int& iy, int& iz) {
  const int64_t q = c / res;                 // < res^2 <= 2^30: 32-bit from here on
  iz = (int)(c - q * res);
  iy = (int)((unsigned)q % (unsigned)res);
  ix = (int)((unsigned)q / (unsigned)res);
}

}  // namespace nerf
