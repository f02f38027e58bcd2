// The hash grid's cell arithmetic for every kernel of hashgrid.hip: the per-axis normalisation (cell_axes, and
// once more inside corners_of: see there), the eight corners, the gathers, the blend, the operand-image store and the corner sums
// of the position gradient.  A change here is a change to all five gather kernels (hash_fwd_kernel, hash_fwd_counted_kernel, hash_fwd_lattice_kernel,
// hash_bwd_input_kernel, hash_bwd_input_ordered_kernel) and to the Corner the scatter kernels consume.
// The normalisation is made of add_rn / mul_rn / sub_rn, divisions and floorf only; the sums below it are plain expressions that
// hipcc contracts under its default -ffp-contract=fast: include this header only in a file compiled that way (hashgrid.hip).
#pragma once
#include "common.h"

namespace nerf {

constexpr int kMaxLevels = 16;

struct HashLevels {
  float scale[kMaxLevels];
  unsigned res[kMaxLevels];
  unsigned size[kMaxLevels];
  unsigned offset[kMaxLevels];
  unsigned dense[kMaxLevels];
  int n_levels;
  float bound;
};

struct Corner {
  unsigned idx[8];
  float w[8];
};

// A point on one level, per axis: the normalised coordinate BEFORE the clamp (the position gradient's clamp test needs it), the
// cell and the position inside it.
struct CellAxes {
  float x01[3];
  unsigned cell[3];
  float frac[3];
};
// HashRepresentation.forward: (x + bound) / (2 bound), clamp to [0, 1]  (embeddings.py:86-87); this is the value before the clamp
__device__ __forceinline__ float box_coordinate(const HashLevels& L, float x) { return add_rn(x, L.bound) / (2.0f * L.bound); }
__device__ __forceinline__ CellAxes cell_axes(const HashLevels& L, int lvl, float px, float py, float pz) {
  CellAxes ax;
  ax.x01[0] = box_coordinate(L, px);
  ax.x01[1] = box_coordinate(L, py);
  ax.x01[2] = box_coordinate(L, pz);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = fminf(fmaxf(ax.x01[a], 0.0f), 1.0f);
    const float pos = add_rn(mul_rn(c, L.scale[lvl]), 0.5f);
    const float fl = floorf(pos);
    ax.frac[a] = sub_rn(pos, fl);
    ax.cell[a] = (unsigned)fl;
  }
  return ax;
}

// The eight corners of the point's cell: table entries and trilinear weights.  The per-axis lines are cell_axes' own, written out
// a second time ON PURPOSE, and every change to one is a change to the other: with corners_of built on cell_axes the compiler lays
// the index code of every caller out differently (same values, same instruction counts), which the ordered input gradient pays
// with 0.3 us of 53.5 at 54 k points -- outside the criterion of DESIGN 4.24.  tests/test_gpu_hashgrid_edges.py holds both to one
// reference: the forward's indices through corners_of, the input gradient's frac and clamp test through cell_axes.
__device__ __forceinline__ Corner corners_of(const HashLevels& L, int lvl, float px, float py, float pz) {
  const float two_b = 2.0f * L.bound;
  float x01[3] = {add_rn(px, L.bound) / two_b, add_rn(py, L.bound) / two_b, add_rn(pz, L.bound) / two_b};
  unsigned cell[3];
  float frac[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = fminf(fmaxf(x01[a], 0.0f), 1.0f);
    const float pos = add_rn(mul_rn(c, L.scale[lvl]), 0.5f);
    const float fl = floorf(pos);
    frac[a] = sub_rn(pos, fl);
    cell[a] = (unsigned)fl;
  }
  Corner out;
  const unsigned res = L.res[lvl], size = L.size[lvl];
  const bool pow2 = (size & (size - 1)) == 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const unsigned gx = cell[0] + (c & 1), gy = cell[1] + ((c >> 1) & 1), gz = cell[2] + ((c >> 2) & 1);
    const float wx = (c & 1) ? frac[0] : sub_rn(1.0f, frac[0]);
    const float wy = (c & 2) ? frac[1] : sub_rn(1.0f, frac[1]);
    const float wz = (c & 4) ? frac[2] : sub_rn(1.0f, frac[2]);
    out.w[c] = mul_rn(mul_rn(wx, wy), wz);
    unsigned e;
    if (L.dense[lvl]) {
      // (gx + gy res + gz res^2) % size: every coordinate is at most res and size >= res^3, so the index is below 2 size --
      // one conditional subtraction gives the remainder (a runtime udiv costs ~30 VALU ops per corner)
      e = gx + gy * res + gz * res * res;
      e = e >= size ? e - size : e;
    }
    else {
      const unsigned h = (gx * 1u) ^ (gy * 2654435761u) ^ (gz * 805459861u);
      e = pow2 ? (h & (size - 1)) : (h % size);     // same value; a runtime udiv costs ~30 VALU ops per corner
    }
    out.idx[c] = e + L.offset[lvl];
  }
  return out;
}

// TableT = float2: the fp32 parameters themselves.  TableT = half2_t: an fp16 copy kept by the optimiser
// (nerf_adamw_clip_step_shadow) -- half the bytes per gather and twice the entries per cache line; tinycudann
// itself evaluates its grid from fp16 parameters next to an fp32 master copy.
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 table_entry(const float2* t, unsigned i) { return t[i]; }
__device__ __forceinline__ float2 table_entry(const half2_t* t, unsigned i) {
  const half2_t h = t[i];
  return make_float2((float)h[0], (float)h[1]);
}
// Which (level, point chunk) a workgroup of the gather kernels works on.  n_chunks > 0 -- XCD-aware 1-D launch of
// 8 * ceil(n_levels / 8) * n_chunks workgroups: the hardware deals consecutive workgroup ids to the eight XCDs in turn, so
// workgroup b runs on XCD b % 8; it takes level (b % 8) + 8 * ((b / 8) / n_chunks), i.e. EVERY lookup into the tables of levels
// x and x + 8 goes through the L2 of XCD x: one hashed level (2 MB of fp16 entries) and one coarse level per 4-MB L2, each
// table fetched from HBM once per launch instead of once per XCD (level-major 2-D launch: 335 MB fetched for 105 MB of
// gathers on 200 k points).  n_chunks == 0: the 2-D launch (blockIdx.y = level).
struct LevelChunk { int lvl, chunk, chunks; };
__device__ __forceinline__ LevelChunk level_chunk(int n_levels, int n_chunks) {
  if (n_chunks <= 0) return {(int)blockIdx.y, (int)blockIdx.x, (int)gridDim.x};
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  return {xcd + 8 * (j / n_chunks), j % n_chunks, n_chunks};
}
inline dim3 level_chunk_grid(int n_levels, int64_t blocks, bool xcd_aware) {
  return xcd_aware ? dim3((unsigned)(8 * ((n_levels + 7) / 8) * blocks)) : dim3((unsigned)blocks, (unsigned)n_levels);
}

// The eight entries of a cell, gathered with as few cache-line requests as the addresses allow.  Corners 2j and 2j+1 differ in x
// only: on a dense level their entries are neighbours (e, e + 1), on a hashed level with an even cell x they are e and e ^ 1
// (the hash XORs x in unmultiplied) -- either way one 8-byte (fp16 table) / 16-byte (fp32) load at min(e0, e1) returns both.
// Otherwise (hashed level, odd x: the carry changes higher bits) the second corner takes its own load.  The gather kernels are
// bound by the texture path's line rate (one 64-byte line per lane and request on the hashed levels), not by bytes.
struct half2x2 { half2_t a, b; };
__device__ __forceinline__ void table_pair(const float2* t, unsigned lo, float2& v0, float2& v1) {
  float4 q;
  __builtin_memcpy(&q, reinterpret_cast<const char*>(t + lo), 16);      // 8-byte aligned: two dwordx2 or one dwordx4
  v0 = make_float2(q.x, q.y);
  v1 = make_float2(q.z, q.w);
}
__device__ __forceinline__ void table_pair(const half2_t* t, unsigned lo, float2& v0, float2& v1) {
  half2x2 q;
  __builtin_memcpy(&q, reinterpret_cast<const char*>(t + lo), 8);       // 4-byte aligned dwordx2
  v0 = make_float2((float)q.a[0], (float)q.a[1]);
  v1 = make_float2((float)q.b[0], (float)q.b[1]);
}
template <class TableT>
__device__ __forceinline__ void gather_cell(const TableT* __restrict__ table, const Corner& c, float2 (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned e0 = c.idx[2 * j], e1 = c.idx[2 * j + 1], lo = e0 < e1 ? e0 : e1;
    if ((e0 > e1 ? e0 - e1 : e1 - e0) == 1u) {
      float2 p0, p1;
      table_pair(table, lo, p0, p1);                       // entries lo and lo + 1 = the two corners
      v[2 * j] = e0 == lo ? p0 : p1;
      v[2 * j + 1] = e0 == lo ? p1 : p0;
    } else {
      v[2 * j] = table_entry(table, e0);
      v[2 * j + 1] = table_entry(table, e1);
    }
  }
}

// The two features of a cell: its eight entries blended with the corner weights.
template <class TableT>
__device__ __forceinline__ float2 cell_features(const TableT* __restrict__ table, const Corner& c) {
  float f0 = 0.0f, f1 = 0.0f;
  float2 v[8];
  gather_cell(table, c, v);
#pragma unroll
  for (int k = 0; k < 8; ++k) {                           // the sums run over the corners in the reference's order
    f0 += c.w[k] * v[k].x;
    f1 += c.w[k] * v[k].y;
  }
  return make_float2(f0, f1);
}

// Rows of an operand image beyond its n (> 0) points, up to the 128-row tile, repeat the last point, so that every stashed value
// is finite (their gradients are zero downstream): the point that row p evaluates.
__device__ __forceinline__ int64_t pad_row(int64_t p, int64_t n) { return p < n ? p : n - 1; }

// Features 2 lvl and 2 lvl + 1 of row p into the natural-order operand blocks of the decoder chains:
// [wave tile of 32 points][k-step ks = level/8][lane (c, h)][8] with feature 16ks + 8h + j; bf16, or fp16 (the Part 4 forward
// chains contract fp16 operands).
__device__ __forceinline__ void store_operand(__bf16* __restrict__ out_nat, int64_t p, int lvl, int n_levels, float f0, float f1, bool fp16) {
  const int f = 2 * lvl, ks = f >> 4, h = (f >> 3) & 1, j = f & 7;
  const int64_t wt = p >> 5;
  const int col = (int)(p & 31);
  const int n_ks = (2 * n_levels + 15) / 16;
  __bf16* dst = out_nat + ((wt * n_ks + ks) * 64 + 2 * col + h) * 8 + j;
  if (fp16) {
    reinterpret_cast<_Float16*>(dst)[0] = (_Float16)f0;
    reinterpret_cast<_Float16*>(dst)[1] = (_Float16)f1;
  } else {
    dst[0] = (__bf16)f0;
    dst[1] = (__bf16)f1;
  }
}

// The cell's part of the gradient with respect to the ENCODED POSITION, from the level's two feature gradients (g0, g1):
//   d[a] = sum_corners (g . table[corner]) * (+1 | -1 along a) * prod_{b != a} w_b,  w = frac | 1 - frac  (cell_axes' frac),
// still to be multiplied by scale_l / (2 bound) (d x01 / d x inside the box) and dropped where HashRepresentation's clamp is
// active.  These are plain expressions: the compiler contracts them, and it does so per caller -- which is why the scale, the
// clamp test and the early-out stay in the two kernels (moved in here, both kernels' last bits change).
template <class TableT>
__device__ __forceinline__ void cell_position_gradient(const TableT* __restrict__ table, const Corner& c, const float (&frac)[3], float g0,
                                                       float g1, float (&d)[3]) {
  d[0] = d[1] = d[2] = 0.0f;
  float2 tv[8];
  gather_cell(table, c, tv);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float2 v = tv[k];
    const float gv = g0 * v.x + g1 * v.y;
    const float wx = (k & 1) ? frac[0] : 1.0f - frac[0], wy = (k & 2) ? frac[1] : 1.0f - frac[1], wz = (k & 4) ? frac[2] : 1.0f - frac[2];
    d[0] += gv * ((k & 1) ? 1.0f : -1.0f) * wy * wz;
    d[1] += gv * ((k & 2) ? 1.0f : -1.0f) * wx * wz;
    d[2] += gv * ((k & 4) ? 1.0f : -1.0f) * wx * wy;
  }
}

}  // namespace nerf
