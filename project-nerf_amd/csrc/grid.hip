// Occupancy-grid refresh helpers (reference src/renderer.py:35-132):
// lattice generation and the overwrite / running-max + threshold + active count pass.
#include "common.h"
#include "lattice.h"
#include "slab_chain.h"

namespace nerf {

__global__ void __launch_bounds__(256)
lattice_kernel(float bound, int res, float step, float* __restrict__ out) {
  const int64_t total = (int64_t)res * res * res;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int iz = (int)(g % res), iy = (int)((g / res) % res), ix = (int)(g / ((int64_t)res * res));
    out[g * 3 + 0] = lattice_node(ix, res, bound, step);   // 'ij' meshgrid, x slowest (renderer.py:53-54)
    out[g * 3 + 1] = lattice_node(iy, res, bound, step);
    out[g * 3 + 2] = lattice_node(iz, res, bound, step);
  }
}

__global__ void __launch_bounds__(256)
grid_update_kernel(const float* __restrict__ cur, float* __restrict__ grid, uint8_t* __restrict__ binary,
                   int64_t n, float decay, int dynamic, float threshold, unsigned long long* __restrict__ count) {
  unsigned long long local = 0;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    float v = cur[g];
    if (dynamic) v = fmaxf(grid[g] * decay, v);          // renderer.py:122-125
    grid[g] = v;
    const bool on = v > threshold;
    binary[g] = on ? 1 : 0;
    local += on ? 1 : 0;
  }
  // one atomic per wave
  for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(count, local);
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_grid_lattice(float bound, int resolution, float* pts_out, nerf_stream_t stream) {
  NERF_REQUIRE(bound > 0.0f && resolution >= 2 && pts_out, "nerf_grid_lattice: bad arguments");
  const float step = lattice_step(bound, resolution);
  hipLaunchKernelGGL(lattice_kernel, dim3(2048), dim3(256), 0, as_stream(stream), bound, resolution, step, pts_out);
  return check_launch("nerf_grid_lattice");
}

extern "C" int nerf_grid_update(const float* sigma, float* grid, uint8_t* binary_grid, int64_t n_cells,
                                float decay, int dynamic, float threshold, unsigned long long* active_count,
                                nerf_stream_t stream) {
  NERF_REQUIRE(n_cells > 0 && sigma && grid && binary_grid && active_count, "nerf_grid_update: bad arguments");
  if (hipMemsetAsync(active_count, 0, sizeof(unsigned long long), as_stream(stream)) != hipSuccess)
    return fail(NERF_ELAUNCH, "nerf_grid_update: memset failed");
  int64_t blocks = (n_cells + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(grid_update_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), sigma, grid, binary_grid,
                     n_cells, decay, dynamic, threshold, active_count);
  return check_launch("nerf_grid_update");
}

// ---- the Instant-NGP field's refresh as one launch chain (reference DensityGrid.update around the hash field,
// src/renderer.py:35-132, the density query src/decoders.py:148-153) ----
// The slab chain of slab_chain.h with ONE pass per slab: hash gather (points from the cell index, or from `pts`) -> sigma-net chain
// with nerf_grid_update's fold in its epilogue.  The workspace is one slab's bf16 operand image.  2 enqueues per slab.
static const size_t kImageRowBytes = 32 * 2;             // 16 levels x 2 features, bf16 or fp16

extern "C" size_t nerf_instant_grid_update_workspace_bytes(int64_t slab_cells) {
  size_t o = 0;
  piece(&o, slab_rows(slab_cells) * kImageRowBytes);
  return o;
}

extern "C" int nerf_instant_grid_update(const void* packed, const float* table_f32, const void* table_f16, int n_levels,
                                        const float* scale_host, const unsigned* res_host, const unsigned* size_host,
                                        const unsigned* offset_host, const unsigned* dense_host, float hash_bound, const float* pts,
                                        int64_t n_cells, int resolution, float grid_bound, float* grid, uint8_t* binary_grid, float decay,
                                        int dynamic, float threshold, unsigned long long* active_count, int64_t slab_cells,
                                        void* workspace, nerf_stream_t stream) {
  static const char* const what = "nerf_instant_grid_update";
  NERF_REQUIRE(n_cells >= 0, "%s: n_cells=%lld", what, (long long)n_cells);
  if (pts != nullptr) {
    NERF_REQUIRE(resolution == 0, "%s: resolution=%d with a point buffer (must be 0)", what, resolution);
    if (n_cells == 0) return NERF_OK;
  } else {
    const int ok = slab_lattice_check(what, resolution, n_cells, grid_bound);
    if (ok != NERF_OK) return ok;
  }
  NERF_REQUIRE(n_levels == 16, "%s: n_levels=%d (the default-shape sigma-net reads 16 levels x 2 features)", what, n_levels);
  NERF_REQUIRE((table_f32 == nullptr) != (table_f16 == nullptr), "%s: exactly one of table_f32 / table_f16", what);
  NERF_REQUIRE(hash_bound > 0.0f, "%s: hash_bound must be positive", what);
  NERF_REQUIRE(packed && scale_host && res_host && size_host && offset_host && dense_host, "%s: NULL pointer", what);
  const LevelArgs levels{n_levels, scale_host, res_host, size_host, offset_host, dense_host, hash_bound};
  return slab_chain(what, n_cells, grid, binary_grid, decay, active_count, slab_cells, workspace, 1, stream,
                    [=](int, int64_t c0, int64_t n, float* slab_grid, uint8_t* slab_binary, float slab_decay, unsigned long long* count) {
                      const int rc = pts != nullptr
                                         ? nerf_hash_encode_fwd_nat(pts + c0 * 3, n, table_f32, table_f16, n_levels, scale_host, res_host, size_host,
                                                                    offset_host, dense_host, hash_bound, workspace, 0, stream)
                                         : hash_fwd_lattice(c0, n, resolution, grid_bound, table_f32, table_f16, levels, workspace, 0, stream);
                      if (rc != NERF_OK) return rc;
                      return imlp_sigma_grid(packed, workspace, n, slab_grid, slab_binary, slab_decay, dynamic, threshold, count, stream);
                    });
}

// ---- the Part 4 dual-hash field's refresh as one launch chain (reference DensityGrid.update in its dynamic form around
// NeuralField('part4'), src/renderer.py:62-86, 118-132, src/core.py:282-352) ----
// The slab chain of slab_chain.h with one pass per time anchor k (t = 0, 0.5, 1): gather of deformation grid k ALONE at the lattice
// nodes (the triangle weights of an anchor are a unit vector) -> density-only deformation chain (x_c) -> canonical gather at x_c ->
// canonical sigma-net chain with the running maximum in its epilogue.  4 enqueues per (slab, anchor).

// byte offsets into the workspace of the two deforming fields: [fp16 operand image of a deformation grid (Part 4 alone) | x_c fp32 |
// fp16 operand image of the canonical grid] of one slab
struct DeformGridLayout { size_t deform_nat, xc, canon_nat, total; };
static DeformGridLayout deform_grid_layout(int64_t slab_cells, bool deform_image) {
  const size_t rows = slab_rows(slab_cells);
  DeformGridLayout l{};
  size_t o = 0;
  l.deform_nat = piece(&o, deform_image ? rows * kImageRowBytes : 0);
  l.xc = piece(&o, rows * 3 * 4);
  l.canon_nat = piece(&o, rows * kImageRowBytes);
  l.total = o;
  return l;
}

extern "C" size_t nerf_p4_grid_update_workspace_bytes(int64_t slab_cells) { return deform_grid_layout(slab_cells, true).total; }

extern "C" int nerf_p4_grid_update(const void* packed, const float* params_f32, const float* const* tables_f32, const void* const* tables_f16,
                                   int deform_levels, const float* d_scale_host, const unsigned* d_res_host, const unsigned* d_size_host,
                                   const unsigned* d_offset_host, const unsigned* d_dense_host, int canon_levels, const float* c_scale_host,
                                   const unsigned* c_res_host, const unsigned* c_size_host, const unsigned* c_offset_host,
                                   const unsigned* c_dense_host, float hash_bound, int64_t n_cells, int resolution, float grid_bound,
                                   float* grid, uint8_t* binary_grid, float decay, float threshold, unsigned long long* active_count,
                                   int64_t slab_cells, void* workspace, nerf_stream_t stream) {
  static const char* const what = "nerf_p4_grid_update";
  NERF_REQUIRE((tables_f32 == nullptr) != (tables_f16 == nullptr),
               "%s: exactly one of tables_f32 / tables_f16 (the four tables are all fp32 or all fp16)", what);
  for (int k = 0; k < 4; ++k)
    NERF_REQUIRE((tables_f32 != nullptr ? (const void*)tables_f32[k] : tables_f16[k]) != nullptr, "%s: table %d is NULL", what, k);
  NERF_REQUIRE(deform_levels == 12 && canon_levels == 16,
               "%s: deform_levels=%d, canon_levels=%d (the default-shape chains read 12 and 16 levels x 2 features)", what, deform_levels,
               canon_levels);
  NERF_REQUIRE(hash_bound > 0.0f, "%s: hash_bound must be positive", what);
  NERF_REQUIRE(packed && params_f32, "%s: NULL pointer", what);
  NERF_REQUIRE(d_scale_host && d_res_host && d_size_host && d_offset_host && d_dense_host && c_scale_host && c_res_host && c_size_host &&
               c_offset_host && c_dense_host, "%s: NULL level table", what);
  const int ok = slab_lattice_check(what, resolution, n_cells, grid_bound);
  if (ok != NERF_OK) return ok;
  const LevelArgs lv_d{deform_levels, d_scale_host, d_res_host, d_size_host, d_offset_host, d_dense_host, hash_bound};
  const DeformGridLayout l = deform_grid_layout(slab_cells, true);
  char* ws = static_cast<char*>(workspace);
  return slab_chain(
      what, n_cells, grid, binary_grid, decay, active_count, slab_cells, workspace, 3, stream,
      [=](int k, int64_t c0, int64_t n, float* slab_grid, uint8_t* slab_binary, float slab_decay, unsigned long long* count) {
        const float anchors[3] = {0.0f, 0.5f, 1.0f}, anchor = anchors[k];
        float* xc = reinterpret_cast<float*>(ws + l.xc);
        int rc = hash_fwd_lattice(c0, n, resolution, grid_bound, tables_f32 ? tables_f32[k] : nullptr, tables_f16 ? tables_f16[k] : nullptr, lv_d,
                                  ws + l.deform_nat, 1, stream);
        if (rc != NERF_OK) return rc;
        rc = p4_deform_lattice(packed, params_f32, ws + l.deform_nat, anchor, c0, n, resolution, grid_bound, xc, stream);
        if (rc != NERF_OK) return rc;
        rc = nerf_hash_encode_fwd_nat(xc, n, tables_f32 ? tables_f32[3] : nullptr, tables_f16 ? tables_f16[3] : nullptr, canon_levels, c_scale_host,
                                      c_res_host, c_size_host, c_offset_host, c_dense_host, hash_bound, ws + l.canon_nat, 1, stream);
        if (rc != NERF_OK) return rc;
        return p4_canon_sigma_grid(packed, ws + l.canon_nat, anchor, n, slab_grid, slab_binary, slab_decay, threshold, count, stream);
      });
}

// ---- the Part 3 field's refresh (MLP deformation, hash-grid canonical field) as one launch chain (reference run.py:1191-1222: the
// union over 8-16 times through DensityGrid.update(..., decay=1.0), src/renderer.py:87-101, 118-132, around NeuralField('part3'),
// src/core.py:233-281, with the deformation MLP of src/decoders.py:165-195) ----
// The slab chain of slab_chain.h with one pass per time j: deformation chain on the lattice nodes at the scalar time (x_c alone) ->
// canonical gather at x_c -> canonical sigma-net chain with the running maximum in its epilogue.  3 enqueues per (slab, time).
extern "C" size_t nerf_p3_grid_update_workspace_bytes(int64_t slab_cells) { return deform_grid_layout(slab_cells, false).total; }

extern "C" int nerf_p3_grid_update(const void* packed_deform, const void* packed_canon, const float* table_f32, const void* table_f16,
                                   int canon_levels, const float* c_scale_host, const unsigned* c_res_host, const unsigned* c_size_host,
                                   const unsigned* c_offset_host, const unsigned* c_dense_host, float hash_bound, const float* times_host,
                                   int n_times, int64_t n_cells, int resolution, float grid_bound, float* grid, uint8_t* binary_grid,
                                   float decay, float threshold, unsigned long long* active_count, int64_t slab_cells, void* workspace,
                                   nerf_stream_t stream) {
  static const char* const what = "nerf_p3_grid_update";
  NERF_REQUIRE((table_f32 == nullptr) != (table_f16 == nullptr), "%s: exactly one of table_f32 / table_f16", what);
  NERF_REQUIRE(canon_levels == 16, "%s: canon_levels=%d (the default-shape sigma-net reads 16 levels x 2 features)", what, canon_levels);
  NERF_REQUIRE(n_times >= 1 && n_times <= 256, "%s: n_times=%d (1..256)", what, n_times);
  NERF_REQUIRE(times_host != nullptr, "%s: times_host is NULL", what);
  for (int j = 0; j < n_times; ++j) NERF_REQUIRE(__builtin_isfinite(times_host[j]), "%s: times_host[%d] is not finite", what, j);
  NERF_REQUIRE(hash_bound > 0.0f, "%s: hash_bound must be positive", what);
  NERF_REQUIRE(packed_deform && packed_canon, "%s: NULL pointer", what);
  NERF_REQUIRE(c_scale_host && c_res_host && c_size_host && c_offset_host && c_dense_host, "%s: NULL level table", what);
  const int ok = slab_lattice_check(what, resolution, n_cells, grid_bound);
  if (ok != NERF_OK) return ok;
  const DeformGridLayout l = deform_grid_layout(slab_cells, false);
  char* ws = static_cast<char*>(workspace);
  return slab_chain(
      what, n_cells, grid, binary_grid, decay, active_count, slab_cells, workspace, n_times, stream,
      [=](int j, int64_t c0, int64_t n, float* slab_grid, uint8_t* slab_binary, float slab_decay, unsigned long long* count) {
        float* xc = reinterpret_cast<float*>(ws + l.xc);
        int rc = p3_deform_lattice(packed_deform, times_host[j], c0, n, resolution, grid_bound, xc, stream);
        if (rc != NERF_OK) return rc;
        rc = nerf_hash_encode_fwd_nat(xc, n, table_f32, table_f16, canon_levels, c_scale_host, c_res_host, c_size_host, c_offset_host,
                                      c_dense_host, hash_bound, ws + l.canon_nat, 1, stream);
        if (rc != NERF_OK) return rc;
        return p4_canon_sigma_grid(packed_canon, ws + l.canon_nat, times_host[j], n, slab_grid, slab_binary, slab_decay, threshold, count, stream);
      });
}
