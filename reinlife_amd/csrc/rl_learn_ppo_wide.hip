// rl_learn_ppo_wide.hip -- the PPO brain's rollouts (rl_learn_ppo.hip: k_learn_ppo) on WIDE rollouts: 1 .. RL_LEARN_PPO_WIDE_MAX rows,
// split into 32-row tiles that run side by side on otherwise idle CUs, with ONE GAE recursion over the whole rollout; and the on-policy
// draw for such rollouts (rl_learn_rollout_wide).  The tiling is this build's own; the rollout's length is not: PPO.learn() trains on the
// WHOLE list gathered since the last call (Models/PPO.py:136-162), which rl_learn_ppo cannot express once it passes 32 rows.
//
// Reference (ReinLife/Models/PPO.py): as rl_learn_ppo.hip states it -- learn() :136-162, pi / v :101-112, Adam :99.
//
// Coupling.  The rows of a rollout meet in two places per epoch and nowhere else: the GAE recursion adv_t = fl(fl(gl adv_(t+1)) + delta_t),
// which runs backwards through ALL rows (not associative: a sequential chain, no scan, no restart at a tile's edge), and the two means
// (1 / batch of the whole rollout).  So an epoch is two passes over the tiles with a launch boundary between them: the first leaves every
// row's td and delta, the second has every tile run the chain itself, identically, from row batch - 1 down to its own first row, out of an
// LDS copy of all deltas (the weight tile's area, free until the forward pass).
//
// Shape.  A call queues 3 n_steps K + 3 launches on the caller's stream, K = the largest k_epoch among the call's learners (a learner with
// a smaller k_epoch sits out the later epochs); nothing is read back, no launch is cooperative, no workgroup waits for another, no float
// atomics.  Every learner has a work buffer, T = ceil(batch / 32):
//   a 64-byte header | lsum[T][2] (double) | td[32 T] | delta[32 T] | partial[T][107,529]        64 + T (16 + 256 + 430,116) bytes
//   k_pwide_check     grid (n_learners), once.  The gate (*fresh == 0: no update, no slot check) and the ring size as k_learn_ppo computes
//                     them; every slot of a call that trains is range-checked (a bad one: error-flag code 6, first in table order); the
//                     header gets {trains, bad, steps taken, calls made, size} AS READ AT ENTRY.  Later kernels read only the header; a
//                     learner marked bad or not training is left alone by the per-epoch kernels.
//   k_pwide_forward   grid (T, n_learners), per rollout s and epoch.  Tile t holds rollout rows 32 t .. min(32 t + 31, batch - 1); rows
//                     beyond the batch are zero rows.  k_learn_ppo's LDS map and arithmetic, thread for thread: the trunk and fc_v on s',
//                     then on s; td and delta of the tile's rows go to the work buffer.  A row's forward arithmetic is k ascending whatever
//                     its place in a tile: its delta does not depend on the tiling.
//   k_pwide_backward  grid (T, n_learners), per rollout and epoch.  The chain (one thread, float32, one multiply and one add per row, no
//                     fma) from row batch - 1 to the tile's first row; the tile's s forward again with both heads (the same bits: the
//                     parameters are only read in these two kernels); k_learn_ppo's per-row scalars, losses and backward pass with
//                     1 / (float)batch of the WHOLE rollout.  Where k_learn_ppo hands a parameter's gradient to Adam, the tile stores it to
//                     partial[t]; the double sums of its rows' two loss terms (rows ascending) go to lsum[t].
//   k_pwide_apply     grid (ceil(n_params / 256), n_learners), per rollout and epoch, one thread per parameter: g = (float)(sum_t (double)
//                     partial[t][i]), t ascending, then rl_learn_dev.h's adam_update with t_adam = steps at entry + s k_epoch + ep + 1;
//                     one thread adds lsum in tile order from 0.0 and writes loss[s][ep].  With one tile every double sum is the round trip
//                     float -> double -> float of one number: batch <= 32 is rl_learn_ppo.
//   k_pwide_finish    once: state[0] += k_epoch per rollout trained, state[1] += 1.
//   packing           rl_learn_merge.hip's k_pack_device, skipping a learner marked bad.
#include "rl_learn_dev.h"

#include <math.h>

int rl_learn_wide_pack_launch(const rl_learner*, int, const long long* const*, hipStream_t);   // rl_learn_merge.hip

namespace {

constexpr int kPBlock = 512;
constexpr int kPRows = 32;                     // rows of a tile (k_learn_ppo's rollout)
constexpr int kPS = 160, kPH = 256;            // LDS row strides in floats (153 / 256 used; columns 153..159 of S are zero)
constexpr int kPWTS = 36;                      // row stride of a forward weight tile [256][32]
constexpr int kPWTFloats = 256 * kPWTS;        // (>= the backward tile's 32 * 256, d1's 32 * 256 and the chain's deltas)
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
constexpr int kRolloutSite = RL_SITE_LEARN_ROLLOUT;
constexpr int kApplyBlock = 256;
constexpr int kMaxTiles = RL_LEARN_PPO_WIDE_MAX / kPRows;
// state-dict-flat offsets (fc1, fc2, fc_pi, fc_v: weight then bias each)
constexpr int oW1 = 0, oB1 = 153 * 256, oW2 = oB1 + 256, oB2 = oW2 + 256 * 256, oWp = oB2 + 256, oBp = oWp + 8 * 256, oWv = oBp + 8,
              oBv = oWv + 256, kNParams = oBv + 1;
static_assert(kNParams == 107529, "the PPO network has 107,529 parameters");
constexpr int kNHead = kNParams - oWp;         // fc_pi.weight, fc_pi.bias, fc_v.weight, fc_v.bias: contiguous, 2,313
constexpr int kHeadRegs = (kNHead + kPBlock - 1) / kPBlock;
static_assert(RL_PPO_ROLLOUT_MAX == kPRows, "a tile is k_learn_ppo's rollout");
static_assert(kMaxTiles * kPRows <= kPWTFloats, "the chain's deltas live in the weight tile");
// the work buffer
constexpr int kHdrBytes = 64;
enum { kHdrTrain = 0, kHdrBad = 1, kHdrSteps = 2, kHdrCalls = 3, kHdrSize = 4 };

struct PWideBrain {
    float *params, *adam_m, *adam_v;
    long long* state;
    float* loss;
    float* grad;
    const float *r_state, *r_state_prime, *r_reward, *r_prob;
    const int8_t* r_action;
    const uint8_t* r_done;
    const unsigned long long* r_count;
    const unsigned long long* fresh;   // rl_ppo.fresh or null
    long long r_capacity;
    char* work;
    double lr, beta1, beta2, eps_d;    // the decimal values the caller's floats stand for (learn_decimal)
    float gamma, gl, clip_lo, clip_hi; // gl = (float)(gamma * lmbda), the bounds (float)(1 -+ eps_clip): from the decimals, as Python makes them
    int k_epoch;
};
struct PWideArgs {
    PWideBrain b[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;              // [n_learners][n_steps][batch]
    int32_t* err;
    int n_steps, batch, tiles;
    int step, epoch;                   // the per-epoch kernels: the rollout and the epoch of this launch
};
static_assert(sizeof(PWideArgs) <= 4096, "the kernels' arguments");

__device__ inline long long* work_hdr(const PWideBrain& B) { return (long long*)B.work; }
__device__ inline double* work_lsum(const PWideBrain& B) { return (double*)(B.work + kHdrBytes); }                     // [T][2]
__device__ inline float* work_td(const PWideBrain& B, int tiles) { return (float*)(work_lsum(B) + 2 * (size_t)tiles); }   // [32 T]
__device__ inline float* work_delta(const PWideBrain& B, int tiles) { return work_td(B, tiles) + (size_t)tiles * kPRows; } // [32 T]
__device__ inline float* work_partial(const PWideBrain& B, int tiles) { return work_delta(B, tiles) + (size_t)tiles * kPRows; }

constexpr int kPLdsFloats = kPRows * kPS + 2 * kPRows * kPH + kPWTFloats + kPRows * 8 * 2 + 12 * kPRows;
constexpr int kPLdsBytes = kPLdsFloats * 4;
static_assert(kPLdsBytes + 1024 <= 160 * 1024, "the tile kernels' LDS map must fit a workgroup's 160 KiB");

__global__ __launch_bounds__(kApplyBlock) void k_pwide_check(const PWideArgs A)
{
    __shared__ int first_bad;
    const int tid = threadIdx.x, brain = blockIdx.x;
    const PWideBrain& B = A.b[brain];
    const int batch = A.batch, n_steps = A.n_steps;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const bool train = !(B.fresh && *B.fresh == 0ull);   // `if self.data()` (PPO.py:76): an empty window makes no update
    int bad = 0x7fffffff;
    const int32_t* sl = A.slots + (size_t)brain * n_steps * batch;
    if (train) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        for (long long i = tid; i < (long long)n_steps * batch; i += kApplyBlock)
            if (sl[i] < 0 || sl[i] >= size) atomicMin(&first_bad, (int)i);
        __syncthreads();
        bad = first_bad;
    }
    if (tid == 0) {
        if (bad != 0x7fffffff && A.err && atomicCAS(A.err, 0, kErrLearnSlot) == 0) { A.err[1] = brain; A.err[2] = bad / batch; A.err[3] = sl[bad]; }
        long long* hdr = work_hdr(B);
        hdr[kHdrTrain] = train ? 1 : 0;
        hdr[kHdrBad] = bad != 0x7fffffff ? 1 : 0;
        hdr[kHdrSteps] = B.state[0];
        hdr[kHdrCalls] = B.state[1];
        hdr[kHdrSize] = size;
        hdr[5] = hdr[6] = hdr[7] = 0;
    }
}

// ---- k_learn_ppo's device code (rl_learn_ppo.hip), copied: that file stays byte for byte what it is ----

// H[row][f] = relu(bias[f] + sum_k W[f][k] X[row][k]), k ascending, for the 32 rows and 256 features.  A thread owns rows 4 rg .. 4 rg + 3
// and features fg, fg + 64, fg + 128, fg + 192; W [256][NIN] row-major comes through the tile wt [256][36] in chunks of 32 k (zero beyond
// NIN: X's padding columns are zero too).  Ends with a barrier.
template <int NIN, int XS>
__device__ __forceinline__ void ppo_forward(const float* W, const float* bias, const float* X, float* H, float* wt, int tid)
{
    const int fg = tid & 63, rg = tid >> 6;
    const int kk = tid & 31, f0 = tid >> 5;    // staging: lane -> k, 16 features per pass
    float acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float b = bias[fg + 64 * j];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r][j] = b;
    }
    float nx[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) nx[p] = kk < NIN ? W[(f0 + 16 * p) * NIN + kk] : 0.0f;
    for (int k0 = 0; k0 < NIN; k0 += 32) {
        __syncthreads();   // the tile is free (and X is complete)
#pragma unroll
        for (int p = 0; p < 16; ++p) wt[(f0 + 16 * p) * kPWTS + kk] = nx[p];
        __syncthreads();
        if (k0 + 32 < NIN) {
#pragma unroll
            for (int p = 0; p < 16; ++p) nx[p] = k0 + 32 + kk < NIN ? W[(f0 + 16 * p) * NIN + k0 + 32 + kk] : 0.0f;
        }
#pragma unroll 2
        for (int k = 0; k < 32; k += 4) {
            f32x4 x[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = *(const f32x4*)(X + (4 * rg + r) * XS + k0 + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = *(const f32x4*)(wt + (fg + 64 * j) * kPWTS + k);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[r][j] = fmaf(w[j].x, x[r].x, acc[r][j]); acc[r][j] = fmaf(w[j].y, x[r].y, acc[r][j]);
                    acc[r][j] = fmaf(w[j].z, x[r].z, acc[r][j]); acc[r][j] = fmaf(w[j].w, x[r].w, acc[r][j]);
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) H[(4 * rg + r) * kPH + fg + 64 * j] = fmaxf(acc[r][j], 0.0f);
    __syncthreads();
}

// acc[r][j] = sum_o W[o][4 kg + j] D[4 rg + r][o], o ascending: the backward pass through fc2 (256 x 256).  W comes through the tile
// wt [32][256] in chunks of 32 outputs, each a contiguous 32 KB of the matrix.  Ends with a barrier (the tile is free).
__device__ __forceinline__ void ppo_backward(const float* W, const float* D, float* wt, float (&acc)[4][4], int tid)
{
    const int kg = tid & 63, rg = tid >> 6;
    float nx[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) nx[p] = W[tid + kPBlock * p];
    for (int o0 = 0; o0 < 256; o0 += 32) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 16; ++p) wt[tid + kPBlock * p] = nx[p];
        __syncthreads();
        if (o0 + 32 < 256) {
#pragma unroll
            for (int p = 0; p < 16; ++p) nx[p] = W[(o0 + 32) * 256 + tid + kPBlock * p];
        }
#pragma unroll 2
        for (int o = 0; o < 32; o += 4) {
            f32x4 d[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = *(const f32x4*)(D + (4 * rg + r) * kPH + o0 + o);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 w = *(const f32x4*)(wt + (o + i) * 256 + 4 * kg);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dv = i == 0 ? d[r].x : i == 1 ? d[r].y : i == 2 ? d[r].z : d[r].w;
                    acc[r][0] = fmaf(w.x, dv, acc[r][0]); acc[r][1] = fmaf(w.y, dv, acc[r][1]);
                    acc[r][2] = fmaf(w.z, dv, acc[r][2]); acc[r][3] = fmaf(w.w, dv, acc[r][3]);
                }
            }
        }
    }
    __syncthreads();
}

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending), stored to the tile's partial row (where k_learn_ppo calls adam_update), for
// a layer of 256 outputs.  A work item is 4 outputs x 4 consecutive k; consecutive threads take consecutive k groups.
template <int NIN, int INS>
__device__ __forceinline__ void ppo_wgrad(float* out, const float* D, const float* IN, int tid)
{
    constexpr int NKG = (NIN + 3) / 4;
    for (int item = tid; item < 64 * NKG; item += kPBlock) {
        const int og = item / NKG, kg = item - og * NKG;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kPRows; ++row) {
            const f32x4 d = *(const f32x4*)(D + row * kPH + 4 * og);
            const f32x4 x = *(const f32x4*)(IN + row * INS + 4 * kg);
            acc[0][0] = fmaf(d.x, x.x, acc[0][0]); acc[0][1] = fmaf(d.x, x.y, acc[0][1]); acc[0][2] = fmaf(d.x, x.z, acc[0][2]); acc[0][3] = fmaf(d.x, x.w, acc[0][3]);
            acc[1][0] = fmaf(d.y, x.x, acc[1][0]); acc[1][1] = fmaf(d.y, x.y, acc[1][1]); acc[1][2] = fmaf(d.y, x.z, acc[1][2]); acc[1][3] = fmaf(d.y, x.w, acc[1][3]);
            acc[2][0] = fmaf(d.z, x.x, acc[2][0]); acc[2][1] = fmaf(d.z, x.y, acc[2][1]); acc[2][2] = fmaf(d.z, x.z, acc[2][2]); acc[2][3] = fmaf(d.z, x.w, acc[2][3]);
            acc[3][0] = fmaf(d.w, x.x, acc[3][0]); acc[3][1] = fmaf(d.w, x.y, acc[3][1]); acc[3][2] = fmaf(d.w, x.z, acc[3][2]); acc[3][3] = fmaf(d.w, x.w, acc[3][3]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * kg + j < NIN) out[(4 * og + i) * NIN + 4 * kg + j] = acc[i][j];
    }
}
__device__ __forceinline__ void ppo_bgrad(float* out, const float* D, int tid)
{
    if (tid < 256) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kPRows; ++row) g += D[row * kPH + tid];
        out[tid] = g;
    }
}

// the tile's rows of `src` (state or state_prime of the ring) -> X [32][160]; rows without a slot and columns >= 153 are zero
__device__ __forceinline__ void ppo_stage_rows(const float* src, const int* row_slot, float* X, int tid)
{
    for (int i = tid; i < kPRows * kPS; i += kPBlock) {
        const int row = i / kPS, k = i - row * kPS, slot = row_slot[row];
        X[i] = (slot >= 0 && k < RL_OBS_DIM) ? src[(size_t)slot * RL_OBS_DIM + k] : 0.0f;
    }
}

// bias + sum_k w[k] h[k], k ascending, over 256 features
__device__ __forceinline__ float ppo_dot256(const float* w, float bias, const float* h)
{
    float acc = bias;
#pragma unroll 4
    for (int k = 0; k < 256; k += 4) {
        const f32x4 x = *(const f32x4*)(h + k);
        acc = fmaf(w[k], x.x, acc); acc = fmaf(w[k + 1], x.y, acc); acc = fmaf(w[k + 2], x.z, acc); acc = fmaf(w[k + 3], x.w, acc);
    }
    return acc;
}

#define PWIDE_LDS_MAP(lds)                                                                                                        \
    float* xs = lds;                                /* S  [32][160] */                                                              \
    float* h1 = xs + kPRows * kPS;                  /* H1 [32][256] */                                                              \
    float* h2 = h1 + kPRows * kPH;                  /* H2 [32][256]  (d2) */                                                        \
    float* wt = h2 + kPRows * kPH;                  /* weight tile (the chain's deltas in front of the forward pass; d1 [32][256]) */ \
    float* lg = wt + kPWTFloats;                    /* [32][8] logits, then dL/dlogit */                                            \
    float* pi = lg + kPRows * 8;                    /* [32][8] softmax */                                                           \
    float* row_v = pi + kPRows * 8;                 /* [32] v(s) */                                                                 \
    float* row_vp = row_v + kPRows;                 /* [32] v(s') */                                                                \
    float* row_r = row_vp + kPRows;                 /* [32] reward / 100 */                                                         \
    float* row_mask = row_r + kPRows;               /* [32] 1 - done */                                                             \
    float* row_pb = row_mask + kPRows;              /* [32] prob_a */                                                               \
    float* row_ratio = row_pb + kPRows;             /* [32] */                                                                      \
    float* row_td = row_ratio + kPRows;             /* [32] */                                                                      \
    float* row_delta = row_td + kPRows;             /* [32] */                                                                      \
    float* row_adv = row_delta + kPRows;            /* [32] */                                                                      \
    float* row_gv = row_adv + kPRows;               /* [32] dL/dv */                                                                \
    float* row_l = row_gv + kPRows;                 /* [32] the row's two loss terms */                                             \
    float* row_l2 = row_l + kPRows;                 /* [32] */

// the per-epoch kernels' common entry: the learner's header says whether this launch has work for it
__device__ __forceinline__ bool pwide_sits_out(const PWideArgs& A, const PWideBrain& B)
{
    const long long* hdr = work_hdr(B);
    return !hdr[kHdrTrain] || hdr[kHdrBad] || A.epoch >= B.k_epoch;   // (uniform) below the gate, a bad slot, or an epoch this learner does not make
}

__global__ __launch_bounds__(kPBlock) void k_pwide_forward(const PWideArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float pwide_lds[];
    PWIDE_LDS_MAP(pwide_lds)
    __shared__ int row_slot[kPRows];

    const int tid = threadIdx.x, tile = blockIdx.x, brain = blockIdx.y;
    const PWideBrain& B = A.b[brain];
    if (pwide_sits_out(A, B)) return;
    const int batch = A.batch, s = A.step;
    const int live = min(kPRows, batch - tile * kPRows);   // the tile's rows inside the rollout (>= 1)
    float* out_td = work_td(B, A.tiles) + tile * kPRows;
    float* out_delta = work_delta(B, A.tiles) + tile * kPRows;
    (void)lg; (void)pi; (void)row_pb; (void)row_ratio; (void)row_td; (void)row_delta; (void)row_adv; (void)row_gv; (void)row_l; (void)row_l2;

    typedef float __attribute__((address_space(1))) gf;   // (the opaque-pointer trick of k_learn_ppo: per-lane parameter addresses are not hoisted and spilled)
    const gf *gP = (const gf*)B.params, *gRS = (const gf*)B.r_state, *gRSP = (const gf*)B.r_state_prime;
    asm volatile("" : "+s"(gP), "+s"(gRS), "+s"(gRSP));
    const float *P = (const float*)gP;
    const float *RS = (const float*)gRS, *RSP = (const float*)gRSP;

    // ---- the tile's rows: rows >= batch are zero rows, and stay out of the chain and of every mean ----
    if (tid < kPRows) {
        const bool in = tid < live;
        const int slot = in ? A.slots[((size_t)brain * A.n_steps + s) * batch + tile * kPRows + tid] : 0;
        row_slot[tid] = in ? slot : -1;
        row_r[tid] = in ? (float)((double)B.r_reward[slot] / 100.0) : 0.0f;   // PPO.py:73
        row_mask[tid] = in ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
    }
    __syncthreads();
    // ---- v(s'): the trunk and fc_v on the s' rows ----
    ppo_stage_rows(RSP, row_slot, xs, tid);
    ppo_forward<153, kPS>(P + oW1, P + oB1, xs, h1, wt, tid);
    ppo_forward<256, kPH>(P + oW2, P + oB2, h1, h2, wt, tid);
    if (tid < kPRows) row_vp[tid] = ppo_dot256(P + oWv, P[oBv], h2 + tid * kPH);
    __syncthreads();
    // ---- v(s): the trunk and fc_v on the s rows (the policy head waits for the second pass) ----
    asm volatile("" : "+s"(gP));   // (opaque again: the first pass's per-lane weight addresses are not kept alive, and spilled, for this one)
    P = (const float*)gP;
    ppo_stage_rows(RS, row_slot, xs, tid);
    ppo_forward<153, kPS>(P + oW1, P + oB1, xs, h1, wt, tid);
    ppo_forward<256, kPH>(P + oW2, P + oB2, h1, h2, wt, tid);
    if (tid < kPRows) {
        const float v = ppo_dot256(P + oWv, P[oBv], h2 + tid * kPH);
        const float td = row_r[tid] + (B.gamma * row_vp[tid]) * row_mask[tid];
        out_td[tid] = td;
        out_delta[tid] = td - v;
    }
    (void)row_v;
}

__global__ __launch_bounds__(kPBlock) void k_pwide_backward(const PWideArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float pwide_lds[];
    PWIDE_LDS_MAP(pwide_lds)
    __shared__ int row_slot[kPRows];
    __shared__ int row_a[kPRows];

    const int tid = threadIdx.x, tile = blockIdx.x, brain = blockIdx.y;
    const PWideBrain& B = A.b[brain];
    if (pwide_sits_out(A, B)) return;
    const int batch = A.batch, s = A.step, tiles = A.tiles;
    const int lo = tile * kPRows;
    const int live = min(kPRows, batch - lo);
    const float* all_td = work_td(B, tiles);
    const float* all_delta = work_delta(B, tiles);
    (void)row_vp; (void)row_r; (void)row_mask; (void)row_delta;

    typedef float __attribute__((address_space(1))) gf;   // (the opaque-pointer trick of k_learn_ppo)
    const gf *gP = (const gf*)B.params, *gRS = (const gf*)B.r_state;
    gf* gPT = (gf*)(work_partial(B, tiles) + (size_t)tile * kNParams);
    asm volatile("" : "+s"(gP), "+s"(gPT), "+s"(gRS));
    const float *P = (const float*)gP, *RS = (const float*)gRS;
    float* PT = (float*)gPT;

    // ---- the tile's rows, and every row's delta into LDS (the weight tile's area: free until the forward pass) ----
    if (tid < kPRows) {
        const bool in = tid < live;
        const int slot = in ? A.slots[((size_t)brain * A.n_steps + s) * batch + lo + tid] : 0;
        row_slot[tid] = in ? slot : -1;
        row_a[tid] = in ? (int)B.r_action[slot] & 7 : 0;
        row_pb[tid] = in ? B.r_prob[slot] : 1.0f;
        row_td[tid] = in ? all_td[lo + tid] : 0.0f;
        row_adv[tid] = 0.0f;
    }
    for (int i = tid; i < batch; i += kPBlock) wt[i] = all_delta[i];
    __syncthreads();
    // ---- GAE, backwards over ALL rows of the rollout from the last one down to this tile's first, no reset at done: float32, one multiply,
    //      one add, no fma (PPO.py:144-150).  Every tile runs the same chain on the same numbers; it keeps the values of its own rows. ----
    if (tid == 0) {
        const float gl = B.gl;
        float adv = 0.0f;
        int t = batch - 1;
#pragma unroll 8
        for (; t >= lo + live; --t) adv = __fadd_rn(__fmul_rn(gl, adv), wt[t]);
        for (; t >= lo; --t) {
            adv = __fadd_rn(__fmul_rn(gl, adv), wt[t]);
            row_adv[t - lo] = adv;
        }
    }
    // ---- the trunk and both heads on the s rows: the bits of k_pwide_forward's (the parameters have not changed since) ----
    ppo_stage_rows(RS, row_slot, xs, tid);
    ppo_forward<153, kPS>(P + oW1, P + oB1, xs, h1, wt, tid);   // (its first barrier completes the chain, in front of the tile's first store)
    ppo_forward<256, kPH>(P + oW2, P + oB2, h1, h2, wt, tid);
    if (tid < kPRows * 8) lg[tid] = ppo_dot256(P + oWp + (tid & 7) * 256, P[oBp + (tid & 7)], h2 + (tid >> 3) * kPH);
    else if (tid < kPRows * 9) row_v[tid - kPRows * 8] = ppo_dot256(P + oWv, P[oBv], h2 + (tid - kPRows * 8) * kPH);
    __syncthreads();
    // ---- softmax and ratio (in double from the f32 logits, rounded once), the losses and dL/dratio, dL/dv per row: one thread per row ----
    if (tid < kPRows) {
        const float* l = lg + tid * 8;
        float mx = l[0];
        for (int a = 1; a < 8; ++a) mx = fmaxf(mx, l[a]);
        double e[8], sum = 0.0;
        for (int a = 0; a < 8; ++a) { e[a] = exp((double)l[a] - (double)mx); sum += e[a]; }
        for (int a = 0; a < 8; ++a) pi[tid * 8 + a] = (float)(e[a] / sum);
        const int a = row_a[tid];
        const float ratio = (float)exp(((double)l[a] - (double)mx - log(sum)) - log((double)row_pb[tid]));
        row_ratio[tid] = ratio;
        const bool in = tid < live;
        const float adv = row_adv[tid];
        const float s1 = ratio * adv;
        const float s2 = fminf(fmaxf(ratio, B.clip_lo), B.clip_hi) * adv;
        const float inside = (ratio >= B.clip_lo && ratio <= B.clip_hi) ? 1.0f : 0.0f;
        const float coef = s1 < s2 ? 1.0f : s2 < s1 ? inside : 0.5f + 0.5f * inside;
        const float gr = in ? -(adv / (float)batch) * coef : 0.0f;   // the mean of the WHOLE rollout
        const float d = row_v[tid] - row_td[tid];
        const float ad = fabsf(d);
        row_l[tid] = in ? -fminf(s1, s2) : 0.0f;
        row_l2[tid] = in ? (ad < 1.0f ? 0.5f * d * d : ad - 0.5f) : 0.0f;
        row_gv[tid] = in ? fminf(fmaxf(d, -1.0f), 1.0f) / (float)batch : 0.0f;
        const float g = gr * ratio;
        for (int j = 0; j < 8; ++j) lg[tid * 8 + j] = in ? g * ((j == a ? 1.0f : 0.0f) - pi[tid * 8 + j]) : 0.0f;
    }
    __syncthreads();
    if (tid == 0) {   // the tile's share of the two means: double sums over its rows, ascending
        double sum = 0.0, sum2 = 0.0;
        for (int j = 0; j < live; ++j) { sum += (double)row_l[j]; sum2 += (double)row_l2[j]; }
        double* ls = work_lsum(B) + 2 * tile;
        ls[0] = sum; ls[1] = sum2;
    }
    // ---- the heads' gradients, into registers: H2 is overwritten next ----
    float head_g[kHeadRegs];
#pragma unroll
    for (int p = 0; p < kHeadRegs; ++p) {
        const int idx = tid + kPBlock * p;
        float g = 0.0f;
        if (idx < 2048) {                      // fc_pi.weight[a][k]
            const int a = idx >> 8, k = idx & 255;
#pragma unroll 4
            for (int row = 0; row < kPRows; ++row) g = fmaf(lg[row * 8 + a], h2[row * kPH + k], g);
        } else if (idx < 2056) {               // fc_pi.bias[a]
            for (int row = 0; row < kPRows; ++row) g += lg[row * 8 + idx - 2048];
        } else if (idx < 2312) {               // fc_v.weight[k]
            const int k = idx - 2056;
#pragma unroll 4
            for (int row = 0; row < kPRows; ++row) g = fmaf(row_gv[row], h2[row * kPH + k], g);
        } else if (idx == 2312) {              // fc_v.bias
            for (int row = 0; row < kPRows; ++row) g += row_gv[row];
        }
        head_g[p] = g;
    }
    __syncthreads();
    // ---- d2 = relu'(h2) * (Wpi^T dlogit + Wv dv), in place ----
    {
        const int k = tid & 255;
        float wa[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) wa[a] = P[oWp + a * 256 + k];
        const float wv = P[oWv + k];
        for (int i = tid; i < kPRows * kPH; i += kPBlock) {
            const int row = i >> 8;
            float sum = 0.0f;
#pragma unroll
            for (int a = 0; a < 8; ++a) sum = fmaf(wa[a], lg[row * 8 + a], sum);
            sum = fmaf(wv, row_gv[row], sum);
            h2[i] = h2[i] > 0.0f ? sum : 0.0f;
        }
    }
    // ---- d1 = relu'(h1) * (W2^T d2), into the weight tile once the pass is through with it ----
    {
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[r][j] = 0.0f;
        ppo_backward(P + oW2, h2, wt, acc, tid);   // (its first barrier completes d2)
        const int kg = tid & 63, rg = tid >> 6;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int at = (4 * rg + r) * kPH + 4 * kg + j;
                wt[at] = h1[at] > 0.0f ? acc[r][j] : 0.0f;
            }
    }
    __syncthreads();
    // ---- the tile's partial gradient, parameter by parameter ----
#pragma unroll
    for (int p = 0; p < kHeadRegs; ++p) {
        const int idx = tid + kPBlock * p;
        if (idx < kNHead) PT[oWp + idx] = head_g[p];
    }
    ppo_wgrad<256, kPH>(PT + oW2, h2, h1, tid);
    ppo_bgrad(PT + oB2, h2, tid);
    ppo_wgrad<153, kPS>(PT + oW1, wt, xs, tid);
    ppo_bgrad(PT + oB1, wt, tid);
}

__global__ __launch_bounds__(kApplyBlock) void k_pwide_apply(const PWideArgs A)
{
    __shared__ double s_bc2_sqrt, s_neg_step;
    const int tid = threadIdx.x;
    const PWideBrain& B = A.b[blockIdx.y];
    if (pwide_sits_out(A, B)) return;
    const long long* hdr = work_hdr(B);
    const int s = A.step, ep = A.epoch, tiles = A.tiles, batch = A.batch;
    const int at = s * B.k_epoch + ep;   // this learner's Adam steps made so far in the call
    if (tid == 0) {
        const double t = (double)(hdr[kHdrSteps] + at + 1);
        s_bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
        s_neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
        if (blockIdx.x == 0 && B.loss) {
            const double* ls = work_lsum(B);
            double sum = 0.0, sum2 = 0.0;
            for (int t2 = 0; t2 < tiles; ++t2) { sum += ls[2 * t2]; sum2 += ls[2 * t2 + 1]; }
            B.loss[at] = (float)(sum / (double)batch + sum2 / (double)batch);
        }
    }
    __syncthreads();
    const int e = blockIdx.x * kApplyBlock + tid;
    if (e >= kNParams) return;
    const float* part = work_partial(B, tiles) + e;
    double sum = 0.0;
#pragma unroll 4
    for (int t = 0; t < tiles; ++t) sum += (double)part[(size_t)t * kNParams];
    AdamStep ad;
    ad.p = B.params; ad.m = B.adam_m; ad.v = B.adam_v;
    ad.grad = B.grad ? B.grad + (size_t)at * kNParams : nullptr;
    ad.w1 = 1.0 - B.beta1; ad.w2 = 1.0 - B.beta2; ad.beta2 = B.beta2; ad.eps = B.eps_d;
    ad.bc2_sqrt = s_bc2_sqrt;
    ad.neg_step = s_neg_step;
    adam_update(ad, e, (float)sum);
}

__global__ __launch_bounds__(64) void k_pwide_finish(const PWideArgs A)
{
    const PWideBrain& B = A.b[blockIdx.x];
    const long long* hdr = work_hdr(B);
    if (hdr[kHdrBad] || threadIdx.x != 0) return;   // a learner marked bad: its buffers stay exactly as they were
    B.state[0] = hdr[kHdrSteps] + (hdr[kHdrTrain] ? (long long)A.n_steps * B.k_epoch : 0);
    B.state[1] = hdr[kHdrCalls] + 1;
}

// ---- rl_learn_rollout_wide: k_rollout_prepare and k_rollout_pick of rl_learn_ppo.hip, copied, with ONE batch of up to
// RL_LEARN_PPO_WIDE_MAX rows for all learners of a call.  Draw d = s * batch + j keeps its salt. ----
struct WRollBrain {
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const int32_t* r_age;
    const unsigned long long* r_count;
    long long r_capacity;
    unsigned long long *keys, *seen, *fresh;
    const long long* state;      // rl_learner.state ([1] = calls made)
};
struct WRollArgs {
    WRollBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* slots;              // [n_learners][n_steps][batch]
    uint64_t seed;
    int n_steps, batch;
};

__device__ inline unsigned long long wrollout_fresh(unsigned long long count, unsigned long long seen, unsigned long long cap)
{
    const unsigned long long f = count > seen ? count - seen : 0ull;
    return f < cap ? f : cap;
}

// one wave per ring row: keys[row] for the rows of the window
__global__ __launch_bounds__(256) void k_wrollout_prepare(const WRollArgs A)
{
    const WRollBrain& B = A.b[blockIdx.y];
    const unsigned long long count = *B.r_count, seen = *B.seen, cap = (unsigned long long)B.r_capacity;
    const unsigned long long fresh = wrollout_fresh(count, seen, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) *B.fresh = fresh;
    const long long size = count < cap ? (long long)count : B.r_capacity;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= size) return;
    const unsigned long long behind = ((unsigned long long)row + cap - (count - fresh) % cap) % cap;   // slots from the window's first to this row's
    if (behind >= fresh) return;   // (wave-uniform)
    const uint64_t k = learn_row_key(B.r_state, B.r_state_prime, B.r_action, B.r_reward, B.r_done, B.r_age, row, lane);
    if (lane == 0) B.keys[row] = k;
}

// one workgroup per draw: slots[brain][d] = the window row with the smallest (mix(key ^ salt_d), slot)
__global__ __launch_bounds__(256) void k_wrollout_pick(const WRollArgs A)
{
    __shared__ uint64_t best_v[256];
    __shared__ int best_i[256];
    const int brain = blockIdx.y, d = blockIdx.x, tid = threadIdx.x;
    const WRollBrain& B = A.b[brain];
    const unsigned long long count = *B.r_count, cap = (unsigned long long)B.r_capacity;
    unsigned long long fresh = *B.fresh;   // (k_wrollout_prepare wrote it in the launch in front of this one)
    if (fresh > cap) fresh = cap;
    if (fresh > count) fresh = count;
    const unsigned long long first = (count - fresh) % cap;
    if (d == 0 && tid == 0) *B.seen = count;   // (k_wrollout_prepare is its only reader)
    const rl_u4 r = rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)B.state[1], (uint32_t)kRolloutSite, (uint32_t)d);
    const uint64_t salt = ((uint64_t)r.y << 32) | r.x;
    uint64_t bv = ~0ull;
    int bi = 0x7fffffff;
    for (unsigned long long j = tid; j < fresh; j += 256) {
        const int i = (int)((first + j) % cap);
        const uint64_t v = learn_mix64(B.keys[i] ^ salt);
        if (v < bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
    best_v[tid] = bv; best_i[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const uint64_t v = best_v[tid + o];
            const int i = best_i[tid + o];
            if (v < best_v[tid] || (v == best_v[tid] && i < best_i[tid])) { best_v[tid] = v; best_i[tid] = i; }
        }
        __syncthreads();
    }
    if (tid == 0) A.slots[(size_t)brain * A.n_steps * A.batch + d] = (fresh > 0 && best_i[0] != 0x7fffffff) ? best_i[0] : 0;
}

}  // namespace

int rl_learn_ppo_wide_supported_impl(int kind) { return kind == RL_PPO ? 1 : 0; }

size_t rl_learn_ppo_wide_work_bytes_impl(int batch)
{
    const size_t tiles = (size_t)(batch + kPRows - 1) / kPRows;
    return kHdrBytes + tiles * (2 * sizeof(double) + 2 * kPRows * sizeof(float) + kNParams * sizeof(float));
}

int rl_learn_ppo_wide_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                             const int32_t* slots, void* const* work, hipStream_t stream)
{
    PWideArgs a{};
    const long long* bad[RL_MAX_CAPTURE_BRAINS];
    int max_k = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        PWideBrain& b = a.b[i];
        b.params = l.params; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_prob = r.prob; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity; b.fresh = ppos[i].fresh;
        b.work = (char*)work[i];
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2); b.eps_d = learn_decimal(l.eps);
        const double gamma = learn_decimal(l.gamma), lmbda = learn_decimal(ppos[i].lmbda), clip = learn_decimal(ppos[i].eps_clip);
        b.gamma = (float)gamma; b.gl = (float)(gamma * lmbda); b.clip_lo = (float)(1.0 - clip); b.clip_hi = (float)(1.0 + clip);
        b.k_epoch = ppos[i].k_epoch;
        max_k = b.k_epoch > max_k ? b.k_epoch : max_k;
        bad[i] = (const long long*)work[i] + kHdrBad;
    }
    a.slots = slots; a.err = h->err_flag; a.n_steps = n_steps;
    a.batch = learners[0].batch; a.tiles = (a.batch + kPRows - 1) / kPRows;
    {   // the large dynamic-LDS window (125 KB), per kernel: asked for at every call -- idempotent, host-only, and right on whatever device is current
        hipError_t e = hipFuncSetAttribute((const void*)k_pwide_forward, hipFuncAttributeMaxDynamicSharedMemorySize, kPLdsBytes);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_pwide_backward, hipFuncAttributeMaxDynamicSharedMemorySize, kPLdsBytes);
        if (e != hipSuccess) { rl_set_error("rl_learn_ppo_wide: hipFuncSetAttribute(%d bytes of LDS) failed: %s", kPLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    const int pblocks = (kNParams + kApplyBlock - 1) / kApplyBlock;
    hipLaunchKernelGGL(k_pwide_check, dim3(n_learners), dim3(kApplyBlock), 0, stream, a);
    for (int s = 0; s < n_steps; ++s)
        for (int ep = 0; ep < max_k; ++ep) {
            a.step = s; a.epoch = ep;
            hipLaunchKernelGGL(k_pwide_forward, dim3(a.tiles, n_learners), dim3(kPBlock), kPLdsBytes, stream, a);
            hipLaunchKernelGGL(k_pwide_backward, dim3(a.tiles, n_learners), dim3(kPBlock), kPLdsBytes, stream, a);
            hipLaunchKernelGGL(k_pwide_apply, dim3(pblocks, n_learners), dim3(kApplyBlock), 0, stream, a);
        }
    hipLaunchKernelGGL(k_pwide_finish, dim3(n_learners), dim3(64), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_ppo_wide: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return rl_learn_wide_pack_launch(learners, n_learners, bad, stream);
}

int rl_learn_rollout_wide_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                                 int32_t* slots, hipStream_t stream)
{
    WRollArgs a{};
    long long max_cap = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        WRollBrain& b = a.b[i];
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done; b.r_age = r.age;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.keys = ppos[i].keys; b.seen = ppos[i].seen; b.fresh = ppos[i].fresh;
        b.state = (const long long*)learners[i].state;
        max_cap = r.capacity > max_cap ? r.capacity : max_cap;
    }
    a.slots = slots; a.seed = h->cfg.seed; a.n_steps = n_steps; a.batch = learners[0].batch;
    hipLaunchKernelGGL(k_wrollout_prepare, dim3((unsigned)((max_cap + 3) / 4), n_learners), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_rollout_wide: launch of the prepare kernel failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    hipLaunchKernelGGL(k_wrollout_pick, dim3((unsigned)(n_steps * a.batch), n_learners), dim3(256), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_rollout_wide: launch of the pick kernel failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}
