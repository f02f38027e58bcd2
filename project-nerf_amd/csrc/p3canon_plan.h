// Compile-time plan of the Part 3 canonical decoder (p3canon.hip): the 8x256 NeRFDecoder of mlp_plan.h on a
// time-conditioned input code [code(x) 63 | code(t) time_dim], time_dim = 1 + 2 L_time <= 21 (reference
// src/core.py:108-113, 233-281).  Same chain, same accumulator / natural k orders and the same 1-KiB A-fragment
// streams as the vanilla plan; only the two steps that read the code are wider:
//   F_PTS0 = {8, 0, 6}, F_PTS4 = {8, 16, 6}: six natural k-steps (96 columns) instead of four.
// Code column j of the reference maps to k = j (j < 63) and to k = 64 + (j - 63) (time code); k = 63 is the
// constant 1 of the vanilla Fourier operand (bias column of the weight gradient), k >= 64 + time_dim is zero.
// The dgrad chain never forms the code's gradient inside the chain, so its stream is the vanilla one
// (plan::kBwdChunks), packed from this layout's offsets.
// This file holds what the layout changes: the parameter Layout, the e* gradient image, code_k / code_col, the two-entry
// step_of override and the pack offsets.  Fragment counts, the chunk table and the m-tile group index come from
// mlp_plan.h's functions, called with this step_of.
#pragma once
#include "mlp_plan.h"

namespace nerf {
namespace cplan {
using plan::Step;
using plan::Chunks;

constexpr int kPosDim = 63, kTimeMax = 21, kCodeK = 96;
constexpr int kCodeKs = 6;                                 // natural k-steps of the code
constexpr int kPlain = plan::kPlain;
constexpr int kTailCount = plan::kParamCount - plan::kWSigma;   // sigma_layer .. rgb_layer, same as vanilla

// k of reference code column j, or -1 past the code
constexpr int code_k(int j, int time_dim) {
  return j < kPosDim ? j : (j - kPosDim < time_dim ? 64 + (j - kPosDim) : -1);
}
// reference code column of k, or -1 (k = 63: the constant column; k beyond the time code: padding)
constexpr int code_col(int k, int time_dim) {
  return k < kPosDim ? k : (k >= 64 && k - 64 < time_dim ? kPosDim + (k - 64) : -1);
}

// ---- reference parameter vector (NeRFDecoder state_dict order, src/decoders.py:37-66) for C = 63 + time_dim ----
struct Layout {
  int C;
  int W0, B0, W1, W4, B4, W5, WSigma, count;
  constexpr int in_dim(int l) const { return l == 0 ? C : (l == 4 ? 256 + C : 256); }
  constexpr int weight_off(int l) const {
    return l == 0 ? W0 : (l < 4 ? W1 + (l - 1) * kPlain : (l == 4 ? W4 : W5 + (l - 5) * kPlain));
  }
  constexpr int bias_off(int l) const { return weight_off(l) + 256 * in_dim(l); }
  // the heads keep the vanilla offsets relative to sigma_layer.weight
  constexpr int tail(int vanilla_off) const { return WSigma + (vanilla_off - plan::kWSigma); }
};
constexpr Layout layout(int time_dim) {
  Layout L{};
  L.C = kPosDim + time_dim;
  L.W0 = 0;
  L.B0 = 256 * L.C;
  L.W1 = L.B0 + 256;
  L.W4 = L.W1 + 3 * kPlain;
  L.B4 = L.W4 + 256 * (256 + L.C);
  L.W5 = L.B4 + 256;
  L.WSigma = L.W5 + 3 * kPlain;
  L.count = L.WSigma + kTailCount;
  return L;
}
static_assert(layout(0).count == plan::kParamCount && layout(0).W4 == plan::kW4, "time_dim 0 is the vanilla vector");
static_assert(layout(21).count == 606596 && layout(13).count == 602500, "parameter counts of the reference's Part 3 decoders");

// ---- weight-gradient image: the wgrad jobs' output, one fixed layout for every time_dim ----
// pts_layers.0 as [256, 96] in k order, pts_layers.4 as its hidden block [256, 256] + bias + code block [256, 96],
// everything else as in the vanilla vector; p3canon.hip's remap kernel gathers it into the reference layout.
constexpr int eW0 = 0, eB0 = 256 * kCodeK, eW1 = eB0 + 256;
constexpr int eW4h = eW1 + 3 * kPlain, eB4 = eW4h + 256 * 256, eW4c = eB4 + 256, eW5 = eW4c + 256 * kCodeK;
constexpr int eWSigma = eW5 + 3 * kPlain, eCount = eWSigma + kTailCount;
constexpr int e_tail(int vanilla_off) { return eWSigma + (vanilla_off - plan::kWSigma); }
constexpr int e_weight_off(int l) { return l < 4 ? eW1 + (l - 1) * kPlain : eW5 + (l - 5) * kPlain; }   // l = 1..3, 5..7

// ---- forward chain steps (plan::Kind numbering) ----
constexpr Step step_of(int kind) {
  if (kind == plan::F_PTS0) return {8, 0, kCodeKs};
  if (kind == plan::F_PTS4) return {8, 16, kCodeKs};
  return plan::step_of(kind);
}
constexpr int kFwdFrags = plan::stream_frags(false, step_of);
static_assert(kFwdFrags == plan::kFwdFrags + 32, "two code steps, two k-steps wider, eight m-tiles each");
constexpr int kBwdFrags = plan::kBwdFrags;
// d code(x) stream of the input gradient: A[j][k] = W0[k][j] (part 0) and W4[k][256 + j] (part 1), code rows j < 64
// (two m-tiles) x 16 accumulator-order k-steps over the 256 hidden units
constexpr int kGradFrags = 2 * 2 * 16;

// the vanilla chunk builder (greedy, m-tile granular, <= 64 fragments) over this step table
constexpr Chunks kFwdChunks = plan::make_chunks(false, step_of);
static_assert(kFwdChunks.n_chunks <= plan::kMaxChunks && kFwdChunks.n_groups <= plan::kMaxGroups, "chunk table size");

// ---- packed buffer (bytes): forward stream | dgrad stream | fp32 bias table (vanilla layout) | d-code stream ----
constexpr size_t kFragBytes = 1024;
constexpr size_t kPackFwdOff = 0;
constexpr size_t kPackBwdOff = kPackFwdOff + (size_t)kFwdFrags * kFragBytes + plan::kStreamPad;
constexpr size_t kPackBiasOff = kPackBwdOff + (size_t)kBwdFrags * kFragBytes + plan::kStreamPad;
constexpr size_t kPackGradOff = kPackBiasOff + ((plan::kBiasFloats * 4 + 255) / 256) * 256;
constexpr size_t kPackBytes = kPackGradOff + (size_t)kGradFrags * kFragBytes;

}  // namespace cplan
}  // namespace nerf
