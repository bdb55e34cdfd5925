// RA-LENet pass: the network's 9 stages and 8 resamplers as ONE node table, the buffers a forward or backward node reads and
// writes derived from its edges, the issue order of a pass, the lane split and the weight-matrix descriptor lists
// (ral_ralenet_plan.hip).  Pure host arithmetic - no HIP call, no stream, no event, usable without a device; the model
// (ral_ralenet.hip) walks the plan and keeps the streams, events and set rotation.  DESIGN.md section 3, "RA-LENet pass".
#pragma once
#include <stdint.h>

#include <vector>

#define RAL_NODES 17
#define RAL_NBLOCKS 18
#define RAL_NRES 8
#ifndef MAX_LANES
#define MAX_LANES 4
#endif

constexpr int CH[5] = {8, 16, 32, 64, 128};   // channel width of a level
constexpr int RWLEN[4] = {32, 16, 8, 4};      // window of R-wave table 1 .. 4

// The named tensors the nodes pass on: the stem's output, the nine stage outputs, the outputs of pm1 .. pm4, the bottleneck's
// x_mid = transformer(p4) + p4 and the outputs of ps4 .. ps1 (u_k: the input of the decoder stage at level k)
enum { RT_NONE = -1, RT_X0 = 0, RT_S0, RT_S1, RT_S2, RT_S3, RT_S4, RT_S5, RT_S6, RT_S7, RT_S8, RT_P1, RT_P2, RT_P3, RT_P4, RT_XMID,
       RT_U3, RT_U2, RT_U1, RT_U0, RT_COUNT };
// The gradient buffers of the workspace, under the names it registers them: gy<b> the gradient of block b's output (gy9 is not a
// buffer: see ralenet_gy), gin<s> of stage s's input, du0 of the head's sum u0 + x0
enum { RG_NONE = -1, RG_GY0 = 0, RG_GIN0 = RAL_NBLOCKS, RG_DU0 = RG_GIN0 + 9, RG_COUNT };
const char* ralenet_tensor_name(int t);          // "x0", "s0" .., "p1" .., "xmid", "u3" ..
void ralenet_grad_name(int g, char out[8]);      // "gy0" .., "gin0" .., "du0"

enum { RN_STAGE = 0, RN_RES = 1 };
struct RalNode {
  int kind, idx;            // RN_STAGE: stage si (blocks 2 si, 2 si + 1); RN_RES: resampler ri
  int level;                // of the node's output
  int rw;                   // stage: its R-wave table 1 .. 4 (0: none)
  int D, up;                // resampler: width of its output, 1 = PatchSeparate (ps), 0 = PatchMerging (pm)
  const char* name;         // prefix in the state dict
  int in, add, out;         // forward edges (RT_*): input; addend (a resampler's skip, the bottleneck's residual); output
};
extern const RalNode RAL_NET[RAL_NODES];         // in forward order
// the head y = transconv(u0 + x0) is no node (the stem and it belong to the caller's stream), but its sum is an edge the rule below reads
constexpr int RAL_HEAD_IN = RT_U0, RAL_HEAD_ADD = RT_X0;
constexpr int RAL_DEC_NODE = 9;                  // first node of the decoder: its first parameter starts gradient bucket 1
const RalNode& ralenet_stage(int si);

// Which buffer holds the gradient of tensor t: gin<s> if stage s reads t, du0 for the head's input, else (t is a stage's own
// output) gy of that stage's second block
int ralenet_grad_of(int t);
// gradient of the output of block blk (0, 1) of stage si: gy<2 si> between the blocks, and the gradient of the node's output
// tensor after the second (gy<2 si + 1>; for the bottleneck, whose output is x_mid, gin5 - there is no gy9)
int ralenet_gy(int si, int blk);
bool ralenet_grad_is_buffer(int g);               // false for gy9 alone: the id names no buffer of the workspace
// a stage's extra: the gradient of the output of the node that takes the stage's input tensor as its addend (RG_NONE: no such node)
int ralenet_extra_of(const RalNode& nd);

// ---- the pass: node entries in issue order; every lane of an entry is issued before the next entry
struct RalPassEntry { int node; bool mark; };    // mark: the decoder bucket events are recorded after this entry
RalPassEntry ralenet_pass(bool backward, int e); // entry e of RAL_NODES
// the buffers of an entry: forward RT_* ids (input, addend, output); backward RG_* ids (dy, extra, dx) and fwd_in, the RT_* id of
// the forward input the node's kernels read again
struct RalBinding { int in, extra, out, fwd_in; };
RalBinding ralenet_bind(const RalNode& nd, bool backward);

// ---- lanes: [0, B) cut into n contiguous micro-batches; B < 64 n or B % n != 0 runs on one lane
struct RalLaneSplit { int n; int w0[MAX_LANES], B[MAX_LANES]; };
RalLaneSplit ralenet_lane_split(int B, int n_lanes);

// ---- parameter offsets (floats into the flat parameter vector; filled by the layout)
struct BlockOff { int64_t wqkv, bqkv, wp, bp, ln1w, ln1b, ln2w, ln2b, w1, b1, w2, b2, le; };
struct ResOff { int64_t w, lnw, lnb; int D; };
struct RalOff {
  int64_t dec_off = 0;   // first float of the decoder's parameters (utransformer4 .. transconv are contiguous up to nparam)
  int64_t conv1_w, conv1_b, bn_w, bn_b, tc_w, tc_b;
  int64_t rw[4] = {-1, -1, -1, -1};
  BlockOff blk[RAL_NBLOCKS];
  ResOff res[RAL_NRES];  // pm1..pm4, ps4..ps1
  bool le = true, rwave = false;
};
// the four weight matrices of a block, shapes in units of its width C
struct BlockMat { int64_t BlockOff::*off; int rows, cols; };
extern const BlockMat BLOCK_MATS[4];
// int4 descriptors {offset, rows, columns, first work item} of every block's matrices (planes_only: of the blocks whose width
// has split planes), as they sit in memory or transposed, then (with_res) of the resamplers' square matrices; a matrix is
// rows * cols / unit_div work items.  Returns the work items in all
int ralenet_mat_descs(const RalOff& O, bool planes_only, bool transposed, int unit_div, bool with_res, std::vector<int>& d);
