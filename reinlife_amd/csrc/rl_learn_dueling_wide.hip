// rl_learn_dueling_wide.hip -- the D3QN brain's minibatch update (rl_learn_dueling.hip: k_learn_d3qn) on WIDE minibatches: 1 ..
// RL_LEARN_DUELING_WIDE_MAX rows, split into 64-row tiles that run side by side on otherwise idle CUs, with the reference's batch-wide
// advantage mean kept exactly.  This build's own: the reference trains one world on ONE minibatch of 64 rows per train() (Models/D3QN.py:
// 97-116); a run of hundreds of worlds appends a thousand times that per learning episode.
//
// Reference (paths under ReinLife/Models):
//   D3QNAgent.train             D3QN.py:97-116   sample, MSE of q[a] against r + gamma (1 - done) max q'_target(s'), ONE Adam step
//   dueling_ddqn.forward        D3QN.py:161-165  q = advantage + value - advantage.mean(): the mean of the WHOLE minibatch's advantages
//
// Coupling.  The rows of a minibatch meet in three scalars per step and nowhere else: M' (the mean of the target network's advantages),
// M (the eval network's) and G = sum_i g_i, which enters dL/dadv[i][a] = g_i [a = a_i] - G / (8 B).  So a step is two
// passes over the tiles with a launch boundary between them: the first leaves each tile's advantage sums and a few numbers per row, the
// second has every tile form the three scalars itself, identically, from those.
//
// Shape.  A call queues 3 n_steps + 3 launches on the caller's stream; nothing is read back, no launch is cooperative, no workgroup waits
// for another, no float atomics.  Every learner has a work buffer, T = ceil(batch / 64):
//   a 64-byte header | partial[T][53,897] | sumA'[T] sumA[T] (padded to 16 bytes) | stash[T][896]
//   stash of tile t: adv'[64][8] | val'[64] | adv[a_i][64] | val[64] | reward[64] | mask[64] | action[64] (int)
//   k_dwide_check     grid (n_learners), once.  Ring size and the gate size > min_size as k_learn_d3qn computes them; every slot of a call
//                     that trains is range-checked (a bad one: error-flag code 6, first in table order); the header gets {trains, bad,
//                     steps taken, calls made, size} AS READ AT ENTRY.  Later kernels read only the header; a learner marked bad or not
//                     training is left alone by the per-step kernels.
//   k_dwide_forward   grid (T, n_learners), per step s.  Tile t holds batch rows 64 t .. min(64 t + 63, batch - 1); rows beyond the batch
//                     are zero rows and stay out of every sum.  k_learn_d3qn's LDS layout and arithmetic, thread for thread: the target
//                     network on s', the eval network on s.  Writes sumA'[t] and sumA[t] (the f32 sum of row_sum[j] over the tile's live
//                     rows, j ascending, by thread 0) and the rows' stash.
//   k_dwide_backward  grid (T, n_learners), per step s.  Every tile: M' = (float)(sum_t (double)sumA'[t]) / (float)(8 batch), t ascending,
//                     M likewise; for ALL rows of the batch, from the stash, k_learn_d3qn's mx, y, q, td and g_i = (2 td) * (1.0f / batch);
//                     per tile the f32 sums of g_i and td^2 over its live rows ascending; G and the loss as double sums over the tiles in
//                     tile order, rounded once.  Then the tile's eval forward again (the same bits: parameters are only read in these two
//                     kernels) and k_learn_d3qn's backward pass with mean_term = G / (float)(8 batch).  Where k_learn_d3qn hands a
//                     parameter's gradient to Adam, the tile stores it to partial[t].  Tile 0 writes loss[s].
//   k_dwide_apply     grid (ceil(n_params / 256), n_learners), per step s, one thread per parameter: g = (float)(sum_t (double)
//                     partial[t][i]), t ascending, then rl_learn_dev.h's adam_update with t_adam = steps at entry + s + 1.  With one tile
//                     every double sum above is the round trip float -> double -> float of one number: batch <= 64 is rl_learn_dueling.
//   k_dwide_finish    once: target <- params where sync_target is set (also below the gate); state[0] += steps made, state[1] += 1.
//   packing           rl_learn_merge.hip's k_pack_device, skipping a learner marked bad.
//
// Prioritised memory (rl_learn_prioritized_wide, RL_PERD3QN).  PERD3QNAgent.train() (PERD3QN.py:94-115) is D3QNAgent.train() plus
// update_priorities(indices, |max_a q'_target(s') - q_eval(s)[a]|) (PERD3QN.py:110-111).  k_dwide_backward<true> and k_dwide_finish<true>
// add exactly that to the <false> instantiations (which compile to what they were): the backward pass already forms the two numbers for
// every row of the batch; the finish pass leaves max(priority[0 .. size)) in *prio_max.  The launches, their grids and the work buffer
// are the same.
#include "rl_learn_dev.h"

int rl_learn_wide_pack_launch(const rl_learner*, int, const long long* const*, hipStream_t);   // rl_learn_merge.hip

namespace {

constexpr int kDBlock = 512;
constexpr int kDRows = 64;                     // rows of a tile
constexpr int kAS = 160, kHS = 128;            // LDS row strides in floats (153 / 128 used; columns 153..159 of A are zero)
constexpr int kWTS = 36;                       // row stride of a forward weight tile [128][32]
constexpr int kWTFloats = 128 * kWTS;          // (>= the backward tile's 32 * 128)
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
constexpr int kLearnSite = RL_SITE_LEARN;
constexpr int kApplyBlock = 256;
constexpr int kMaxTiles = RL_LEARN_DUELING_WIDE_MAX / kDRows;
// state-dict-flat offsets of the dueling network (fc, adv_fc1, adv_fc2, value_fc1, value_fc2: weight then bias each)
constexpr int oW0 = 0, oB0 = 153 * 128, oWa1 = oB0 + 128, oBa1 = oWa1 + 128 * 128, oWa2 = oBa1 + 128, oBa2 = oWa2 + 8 * 128,
              oWv1 = oBa2 + 8, oBv1 = oWv1 + 128 * 128, oWv2 = oBv1 + 128, oBv2 = oWv2 + 128, kNParams = oBv2 + 1;
static_assert(kNParams == 53897, "the dueling network has 53,897 parameters");
constexpr int kNHead = 8 * 128 + 8 + 128 + 1;  // adv_fc2.weight, adv_fc2.bias | value_fc2.weight, value_fc2.bias
// the work buffer
constexpr int kHdrBytes = 64;
enum { kHdrTrain = 0, kHdrBad = 1, kHdrSteps = 2, kHdrCalls = 3, kHdrSize = 4 };
constexpr int kStashFloats = kDRows * 14;      // per tile
constexpr int oSAdvP = 0, oSValP = kDRows * 8, oSAdvA = oSValP + kDRows, oSVal = oSAdvA + kDRows, oSR = oSVal + kDRows, oSMask = oSR + kDRows,
              oSAct = oSMask + kDRows;
static_assert(oSAct + kDRows == kStashFloats, "the stash of a tile");

struct DWideBrain {
    float *params, *target, *adam_m, *adam_v;
    long long* state;
    float* loss;
    float* grad;
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const unsigned long long* r_count;
    long long r_capacity;
    char* work;
    double lr, beta1, beta2, eps_d;   // the decimal values the caller's floats stand for (learn_decimal)
    float gamma;
    int min_size, sync_target;
};

struct DWidePrio {               // the prioritised memory of a brain (the <true> instantiations only: rl_learn_prioritized_wide)
    float* priority;             // [ring capacity]
    float* prio_max;             // [1]
};

struct DWideArgs {
    DWideBrain b[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;        // [n_learners][n_steps][batch] or null
    int32_t* err;
    uint64_t seed;
    int n_steps, batch, tiles;
    int step;                    // the per-step kernels: the step of this launch
    DWidePrio p[RL_MAX_CAPTURE_BRAINS];   // (behind everything else: the fields above sit where they sat)
};

__host__ __device__ inline size_t dwide_sums_bytes(int tiles) { return ((size_t)2 * tiles * sizeof(float) + 15) & ~(size_t)15; }
__device__ inline long long* work_hdr(const DWideBrain& B) { return (long long*)B.work; }
__device__ inline float* work_partial(const DWideBrain& B) { return (float*)(B.work + kHdrBytes); }
__device__ inline float* work_sums(const DWideBrain& B, int tiles) { return work_partial(B) + (size_t)tiles * kNParams; }   // sumA'[T] sumA[T]
__device__ inline float* work_stash(const DWideBrain& B, int tiles) { return (float*)((char*)work_sums(B, tiles) + dwide_sums_bytes(tiles)); }

constexpr int kDLdsFloats = kDRows * kAS + 3 * kDRows * kHS + kWTFloats + kDRows * 8 + 6 * kDRows;
constexpr int kDLdsBytes = kDLdsFloats * 4;
static_assert(kDLdsBytes + 2048 <= 160 * 1024, "the tile kernels' LDS map must fit a workgroup's 160 KiB");
static_assert(2 * kDRows * kHS >= kDRows * kAS, "HA + HV must hold the minibatch's observation rows");
static_assert(2 * (RL_LEARN_DUELING_WIDE_MAX + kMaxTiles) <= kDRows * kHS, "F holds the whole batch's g and td^2 before the forward pass");

__global__ __launch_bounds__(kApplyBlock) void k_dwide_check(const DWideArgs A)
{
    __shared__ int first_bad;
    const int tid = threadIdx.x, brain = blockIdx.x;
    const DWideBrain& B = A.b[brain];
    const int batch = A.batch, n_steps = A.n_steps;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const bool train = size > B.min_size;
    int bad = 0x7fffffff;
    const int32_t* sl = A.slots ? A.slots + (size_t)brain * n_steps * batch : nullptr;
    if (sl && train) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        for (int i = tid; i < n_steps * batch; i += kApplyBlock)
            if (sl[i] < 0 || sl[i] >= size) atomicMin(&first_bad, i);
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

// ---- k_learn_d3qn's device code (rl_learn_dueling.hip), copied: that file stays byte for byte what it is ----

// H[row][f] = relu(bias[f] + sum_k W[f][k] X[row][k]), k ascending, for the 64 rows and 128 features.  A thread owns rows 4 rg .. 4 rg + 3
// and features fg, fg + 32, fg + 64, fg + 96; W [128][NIN] row-major comes through the tile wt [128][36] in chunks of 32 k (zero beyond NIN:
// X's padding columns are zero too).  Ends with a barrier.
template <int NIN, int XS>
__device__ __forceinline__ void duel_forward(const float* W, const float* bias, const float* X, float* H, float* wt, int tid)
{
    const int fg = tid & 31, rg = tid >> 5;
    const int kk = tid & 31, f0 = tid >> 5;    // staging: lane -> k, 16 features per pass
    float acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float b = bias[fg + 32 * j];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r][j] = b;
    }
    float nx[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) nx[p] = kk < NIN ? W[(f0 + 16 * p) * NIN + kk] : 0.0f;
    for (int k0 = 0; k0 < NIN; k0 += 32) {
        __syncthreads();   // the tile is free (and X is complete)
#pragma unroll
        for (int p = 0; p < 8; ++p) wt[(f0 + 16 * p) * kWTS + kk] = nx[p];
        __syncthreads();
        if (k0 + 32 < NIN) {
#pragma unroll
            for (int p = 0; p < 8; ++p) nx[p] = k0 + 32 + kk < NIN ? W[(f0 + 16 * p) * NIN + k0 + 32 + kk] : 0.0f;
        }
#pragma unroll 2
        for (int k = 0; k < 32; k += 4) {
            f32x4 x[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = *(const f32x4*)(X + (4 * rg + r) * XS + k0 + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = *(const f32x4*)(wt + (fg + 32 * j) * kWTS + k);
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
        for (int j = 0; j < 4; ++j) H[(4 * rg + r) * kHS + fg + 32 * j] = fmaxf(acc[r][j], 0.0f);
    __syncthreads();
}

// acc[r][j] += sum_o W[o][4 kg + j] D[4 rg + r][o], o ascending: the backward pass through a 128 x 128 layer.  W comes through the tile
// wt [32][128] in chunks of 32 outputs, each a contiguous 16 KB of the matrix.
__device__ __forceinline__ void duel_backward(const float* W, const float* D, float* wt, float (&acc)[4][4], int tid)
{
    const int kg = tid & 31, rg = tid >> 5;
    float nx[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) nx[p] = W[tid + kDBlock * p];
    for (int o0 = 0; o0 < 128; o0 += 32) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 8; ++p) wt[tid + kDBlock * p] = nx[p];
        __syncthreads();
        if (o0 + 32 < 128) {
#pragma unroll
            for (int p = 0; p < 8; ++p) nx[p] = W[(o0 + 32) * 128 + tid + kDBlock * p];
        }
#pragma unroll 2
        for (int o = 0; o < 32; o += 4) {
            f32x4 d[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = *(const f32x4*)(D + (4 * rg + r) * kHS + o0 + o);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 w = *(const f32x4*)(wt + (o + i) * 128 + 4 * kg);
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

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending), stored to the tile's partial row (where k_learn_d3qn calls adam_update), for
// a layer of 128 outputs.  A work item is 4 outputs x 4 consecutive k; consecutive threads take consecutive k groups.
template <int NIN, int DS, int INS>
__device__ __forceinline__ void duel_wgrad(float* out, const float* D, const float* IN, int tid)
{
    constexpr int NKG = (NIN + 3) / 4;
    for (int item = tid; item < 32 * NKG; item += kDBlock) {
        const int og = item / NKG, kg = item - og * NKG;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kDRows; ++row) {
            const f32x4 d = *(const f32x4*)(D + row * DS + 4 * og);
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
template <int DS>
__device__ __forceinline__ void duel_bgrad(float* out, const float* D, int tid)
{
    if (tid < 128) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kDRows; ++row) g += D[row * DS + tid];
        out[tid] = g;
    }
}

// the tile's rows of `src` (state or state_prime of the ring) -> X [64][160]; rows without a slot and columns >= 153 are zero
__device__ __forceinline__ void duel_stage_rows(const float* src, const int* row_slot, float* X, int tid)
{
    for (int i = tid; i < kDRows * kAS; i += kDBlock) {
        const int row = i / kAS, k = i - row * kAS, slot = row_slot[row];
        X[i] = (slot >= 0 && k < RL_OBS_DIM) ? src[(size_t)slot * RL_OBS_DIM + k] : 0.0f;
    }
}

// The network P on the rows in X: F, HA, HV as rl_learn_dueling.hip's header says, adv [64][8] and val [64] (no mean taken yet),
// row_sum[row] = the row's eight advantages added in action order.  Ends with a barrier.
__device__ __forceinline__ void duel_network(const float* P, const float* X, float* F, float* HA, float* HV, float* wt, float* adv, float* val,
                                    float* row_sum, int tid)
{
    duel_forward<153, kAS>(P + oW0, P + oB0, X, F, wt, tid);
    duel_forward<128, kHS>(P + oWa1, P + oBa1, F, HA, wt, tid);
    duel_forward<128, kHS>(P + oWv1, P + oBv1, F, HV, wt, tid);
    {   // the heads: thread (row, a) makes adv[row][a]; the thread of a = 0 then makes val[row]
        const int row = tid >> 3, a = tid & 7;
        const float* w = P + oWa2 + a * 128;
        float acc = P[oBa2 + a];
#pragma unroll 4
        for (int k = 0; k < 128; k += 4) {
            const f32x4 h = *(const f32x4*)(HA + row * kHS + k);
            acc = fmaf(w[k], h.x, acc); acc = fmaf(w[k + 1], h.y, acc); acc = fmaf(w[k + 2], h.z, acc); acc = fmaf(w[k + 3], h.w, acc);
        }
        adv[tid] = acc;
        if (a == 0) {
            const float* wv = P + oWv2;
            float v = P[oBv2];
#pragma unroll 4
            for (int k = 0; k < 128; k += 4) {
                const f32x4 h = *(const f32x4*)(HV + row * kHS + k);
                v = fmaf(wv[k], h.x, v); v = fmaf(wv[k + 1], h.y, v); v = fmaf(wv[k + 2], h.z, v); v = fmaf(wv[k + 3], h.w, v);
            }
            val[row] = v;
        }
    }
    __syncthreads();
    if (tid < kDRows) {
        float s = adv[tid * 8];
        for (int a = 1; a < 8; ++a) s += adv[tid * 8 + a];
        row_sum[tid] = s;
    }
    __syncthreads();
}

// row j of the WHOLE batch at step s: the caller's table, or rl_learn_dueling's Philox mapping with draw index s * batch + j
__device__ __forceinline__ int dwide_slot(const DWideArgs& A, int brain, int s, int j, long long calls, long long size)
{
    if (A.slots) return A.slots[((size_t)brain * A.n_steps + s) * A.batch + j];
    return (int)(((uint64_t)rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)calls, (uint32_t)kLearnSite, (uint32_t)(s * A.batch + j)).x * (uint64_t)size) >> 32);
}

#define DWIDE_LDS_MAP(lds)                                                                                                        \
    float* xa = lds;                                /* A  [64][160]  (d_f [64][128] during the backward pass) */                    \
    float* fa = xa + kDRows * kAS;                  /* F  [64][128] */                                                              \
    float* ha = fa + kDRows * kHS;                  /* HA [64][128]  (da; with HV: the s rows again for fc's weight gradient) */    \
    float* hv = ha + kDRows * kHS;                  /* HV [64][128]  (dv) */                                                        \
    float* wt = hv + kDRows * kHS;                  /* weight tile */                                                               \
    float* adv = wt + kWTFloats;                    /* [64][8] advantages, then dL/dadv */                                          \
    float* val = adv + kDRows * 8;                  /* [64] */                                                                      \
    float* row_sum = val + kDRows;                  /* [64] a row's advantages added */                                             \
    float* row_g = row_sum + kDRows;                /* [64] dL/dq[a] = 2 td / batch */                                              \
    float* row_r = row_g + kDRows;                  /* [64] reward */                                                               \
    float* row_mask = row_r + kDRows;               /* [64] 1 - done */                                                             \
    float* row_y = row_mask + kDRows;               /* [64] (k_learn_d3qn's max q' / td^2: unused here, the layout is kept) */

__global__ __launch_bounds__(kDBlock) void k_dwide_forward(const DWideArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float dwide_lds[];
    DWIDE_LDS_MAP(dwide_lds)
    __shared__ int row_slot[kDRows];
    __shared__ int row_a[kDRows];

    const int tid = threadIdx.x, tile = blockIdx.x, brain = blockIdx.y;
    const DWideBrain& B = A.b[brain];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform) below the gate, or a bad slot: nothing of this learner is written
    const int batch = A.batch, s = A.step;
    const long long size = hdr[kHdrSize], calls = hdr[kHdrCalls];
    const int live = min(kDRows, batch - tile * kDRows);   // the tile's rows inside the batch (>= 1)
    float* sums = work_sums(B, A.tiles);
    float* stash = work_stash(B, A.tiles) + (size_t)tile * kStashFloats;
    (void)row_g; (void)row_y;

    typedef float __attribute__((address_space(1))) gf;   // (the opaque-pointer trick of k_learn_d3qn: per-lane parameter addresses are not hoisted and spilled)
    gf *gP = (gf*)B.params, *gT = (gf*)B.target;
    const gf *gRS = (const gf*)B.r_state, *gRSP = (const gf*)B.r_state_prime;
    asm volatile("" : "+s"(gP), "+s"(gT), "+s"(gRS), "+s"(gRSP));
    const float *P = (const float*)gP, *T = (const float*)gT;
    const float *RS = (const float*)gRS, *RSP = (const float*)gRSP;

    // ---- the tile's rows: rows >= batch are zero rows, and stay out of the batch-wide mean ----
    if (tid < kDRows) {
        const bool in = tid < live;
        const int slot = in ? dwide_slot(A, brain, s, tile * kDRows + tid, calls, size) : 0;
        row_slot[tid] = in ? slot : -1;
        row_a[tid] = in ? (int)B.r_action[slot] & 7 : 0;
        row_r[tid] = in ? B.r_reward[slot] : 0.0f;
        row_mask[tid] = in ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
    }
    __syncthreads();
    // ---- the target network on s': adv', val' and the tile's share of M' ----
    duel_stage_rows(RSP, row_slot, xa, tid);
    duel_network(T, xa, fa, ha, hv, wt, adv, val, row_sum, tid);
    stash[oSAdvP + tid] = adv[tid];
    if (tid < kDRows) stash[oSValP + tid] = val[tid];
    if (tid == 0) {
        float sum = 0.0f;
        for (int j = 0; j < live; ++j) sum += row_sum[j];
        sums[tile] = sum;
    }
    __syncthreads();
    // ---- the eval network on s: adv[a_i], val and the tile's share of M ----
    duel_stage_rows(RS, row_slot, xa, tid);
    duel_network(P, xa, fa, ha, hv, wt, adv, val, row_sum, tid);
    if (tid < kDRows) {
        stash[oSAdvA + tid] = adv[tid * 8 + row_a[tid]];
        stash[oSVal + tid] = val[tid];
        stash[oSR + tid] = row_r[tid];
        stash[oSMask + tid] = row_mask[tid];
        ((int*)stash)[oSAct + tid] = row_a[tid];
    }
    if (tid == 0) {
        float sum = 0.0f;
        for (int j = 0; j < live; ++j) sum += row_sum[j];
        sums[A.tiles + tile] = sum;
    }
}

// PRIO: the prioritised memory's upkeep (rl_learn_prioritized_wide), as k_learn_d3qn<true> adds it to k_learn_d3qn<false>.  In the all-rows
// loop the thread that handles batch row i = 64 t + r of THIS tile (t == tile, i < batch) writes priority[row_slot[r]] = |mx - q|
// (PERD3QN.py:110-111), from this step's pre-update parameters.  mx and q come from the row's stash entries and from M' and M, which every
// tile forms identically; the forward arithmetic of a row is k ascending whatever its place in a tile: a slot drawn several times, in one
// tile or in several, is written with equal bits, so no winner rule exists.  Padding rows (row_slot = -1) are not in the batch and never
// index priority; k_dwide_check has range-checked every other slot against size <= capacity before this kernel runs.
template <bool PRIO>
__global__ __launch_bounds__(kDBlock) void k_dwide_backward(const DWideArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float dwide_lds[];
    DWIDE_LDS_MAP(dwide_lds)
    __shared__ int row_slot[kDRows];
    __shared__ int row_a[kDRows];
    __shared__ float mean_p, mean_e, batch_G;
    __shared__ float tile_g[kMaxTiles], tile_l[kMaxTiles];

    const int tid = threadIdx.x, tile = blockIdx.x, brain = blockIdx.y;
    const DWideBrain& B = A.b[brain];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform)
    const int batch = A.batch, s = A.step, tiles = A.tiles;
    const long long size = hdr[kHdrSize], calls = hdr[kHdrCalls];
    const int live = min(kDRows, batch - tile * kDRows);
    const float inv_batch = 1.0f / (float)batch;
    const float* sums = work_sums(B, tiles);
    const float* stash = work_stash(B, tiles);
    float* part = work_partial(B) + (size_t)tile * kNParams;
    (void)row_r; (void)row_mask; (void)row_y;

    typedef float __attribute__((address_space(1))) gf;   // (the opaque-pointer trick of k_learn_d3qn: per-lane parameter addresses are not hoisted and spilled)
    gf *gP = (gf*)B.params, *gPT = (gf*)part;
    const gf *gRS = (const gf*)B.r_state;
    asm volatile("" : "+s"(gP), "+s"(gPT), "+s"(gRS));
    const float* P = (const float*)gP;
    float* PT = (float*)gPT;
    const float* RS = (const float*)gRS;

    // ---- the batch scalars, formed by every tile identically: M', M, then g_i and td^2 of ALL rows, then G and the loss ----
    if (tid == 0) {
        double sp = 0.0, se = 0.0;
        for (int t = 0; t < tiles; ++t) { sp += (double)sums[t]; se += (double)sums[tiles + t]; }
        mean_p = (float)sp / (float)(8 * batch);
        mean_e = (float)se / (float)(8 * batch);
    }
    if (tid < kDRows) row_slot[tid] = tid < live ? dwide_slot(A, brain, s, tile * kDRows + tid, calls, size) : -1;
    __syncthreads();
    float* all_g = fa;                                   // [T][65]: the F area is free until the forward pass (a pad word per tile: the
    float* all_l = fa + kMaxTiles * (kDRows + 1);        // tiles' serial sums below read distinct banks)
    for (int i = tid; i < tiles * kDRows; i += kDBlock) {
        const int t = i >> 6, r = i & 63;
        const float* st = stash + (size_t)t * kStashFloats;
        const float m = mean_p, v = st[oSValP + r];
        float mx = (st[oSAdvP + r * 8] + v) - m;
        for (int a = 1; a < 8; ++a) mx = fmaxf(mx, (st[oSAdvP + r * 8 + a] + v) - m);
        const float y = st[oSR + r] + (B.gamma * st[oSMask + r]) * mx;
        const float q = (st[oSAdvA + r] + st[oSVal + r]) - mean_e;
        const float td = q - y;
        const bool in = i < batch;
        const float l = in ? td * td : 0.0f;
        const float g = in ? (2.0f * td) * inv_batch : 0.0f;
        all_l[t * (kDRows + 1) + r] = l;
        all_g[t * (kDRows + 1) + r] = g;
        if (PRIO && t == tile && in) A.p[brain].priority[row_slot[r]] = fabsf(mx - q);   // only a row's own tile writes it
        if (t == tile) { row_g[r] = g; row_a[r] = ((const int*)st)[oSAct + r]; }
    }
    __syncthreads();
    if (tid < tiles) {
        const int n = min(kDRows, batch - tid * kDRows);
        float sum = 0.0f, G = 0.0f;
        for (int j = 0; j < n; ++j) { sum += all_l[tid * (kDRows + 1) + j]; G += all_g[tid * (kDRows + 1) + j]; }
        tile_l[tid] = sum; tile_g[tid] = G;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0, G = 0.0;
        for (int t = 0; t < tiles; ++t) { sum += (double)tile_l[t]; G += (double)tile_g[t]; }
        if (tile == 0 && B.loss) B.loss[s] = (float)sum * inv_batch;
        batch_G = (float)G;
    }
    __syncthreads();
    // ---- the tile's eval forward again: the bits of k_dwide_forward's (the parameters have not changed since) ----
    duel_stage_rows(RS, row_slot, xa, tid);
    duel_network(P, xa, fa, ha, hv, wt, adv, val, row_sum, tid);
    {   // dL/dadv[i][a] = g_i [a = a_i] - G / (8 batch) on the batch's rows (the mean reaches every row and action), zero on padding rows
        const int row = tid >> 3, a = tid & 7;
        const float mean_term = batch_G / (float)(8 * batch);
        adv[tid] = row < live ? (a == row_a[row] ? row_g[row] : 0.0f) - mean_term : 0.0f;
    }
    __syncthreads();
    // ---- the heads' gradients, into registers: HA and HV are overwritten next ----
    float head_g[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int idx = tid + kDBlock * p;
        float g = 0.0f;
        if (idx < 1024) {                      // adv_fc2.weight[a][k]
            const int a = idx >> 7, k = idx & 127;
#pragma unroll 4
            for (int row = 0; row < kDRows; ++row) g = fmaf(adv[row * 8 + a], ha[row * kHS + k], g);
        } else if (idx < 1032) {               // adv_fc2.bias[a]
            for (int row = 0; row < kDRows; ++row) g += adv[row * 8 + idx - 1024];
        } else if (idx < 1160) {               // value_fc2.weight[k]
            const int k = idx - 1032;
#pragma unroll 4
            for (int row = 0; row < kDRows; ++row) g = fmaf(row_g[row], hv[row * kHS + k], g);
        } else if (idx == 1160) {              // value_fc2.bias
            for (int row = 0; row < kDRows; ++row) g += row_g[row];
        }
        head_g[p] = g;
    }
    __syncthreads();
    // ---- backward through the branches' ReLUs, in place: da = relu'(h_adv) * (Wa2^T dadv), dv = relu'(h_val) * Wv2 * g ----
    {
        const int k = tid & 127;
        float wa[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) wa[a] = P[oWa2 + a * 128 + k];
        const float wv = P[oWv2 + k];
        for (int i = tid; i < kDRows * 128; i += kDBlock) {
            const int row = i >> 7;
            float sum = 0.0f;
#pragma unroll
            for (int a = 0; a < 8; ++a) sum = fmaf(wa[a], adv[row * 8 + a], sum);
            ha[i] = ha[i] > 0.0f ? sum : 0.0f;
            hv[i] = hv[i] > 0.0f ? wv * row_g[row] : 0.0f;
        }
    }
    // ---- d_f = relu'(f) * (Wa1^T da + Wv1^T dv), into the A area (s is not needed until fc's weight gradient) ----
    {
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[r][j] = 0.0f;
        duel_backward(P + oWa1, ha, wt, acc, tid);   // (its first barrier completes da / dv)
        duel_backward(P + oWv1, hv, wt, acc, tid);
        const int kg = tid & 31, rg = tid >> 5;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int at = (4 * rg + r) * kHS + 4 * kg + j;
                xa[at] = fa[at] > 0.0f ? acc[r][j] : 0.0f;
            }
    }
    __syncthreads();
    // ---- the tile's partial gradient, parameter by parameter ----
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int idx = tid + kDBlock * p;
        if (idx < 1032) PT[oWa2 + idx] = head_g[p];
        else if (idx < kNHead) PT[oWv2 + idx - 1032] = head_g[p];
    }
    duel_wgrad<128, kHS, kHS>(PT + oWa1, ha, fa, tid);
    duel_bgrad<kHS>(PT + oBa1, ha, tid);
    duel_wgrad<128, kHS, kHS>(PT + oWv1, hv, fa, tid);
    duel_bgrad<kHS>(PT + oBv1, hv, tid);
    __syncthreads();   // HA and HV are free: the s rows come back from the ring
    duel_stage_rows(RS, row_slot, ha, tid);
    __syncthreads();
    duel_wgrad<153, kHS, kAS>(PT + oW0, xa, ha, tid);
    duel_bgrad<kHS>(PT + oB0, xa, tid);
}

__global__ __launch_bounds__(kApplyBlock) void k_dwide_apply(const DWideArgs A)
{
    __shared__ double s_bc2_sqrt, s_neg_step;
    const int tid = threadIdx.x;
    const DWideBrain& B = A.b[blockIdx.y];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform)
    const int s = A.step, tiles = A.tiles;
    if (tid == 0) {
        const double t = (double)(hdr[kHdrSteps] + s + 1);
        s_bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
        s_neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
    }
    __syncthreads();
    const int e = blockIdx.x * kApplyBlock + tid;
    if (e >= kNParams) return;
    const float* part = work_partial(B) + e;
    double sum = 0.0;
#pragma unroll 4
    for (int t = 0; t < tiles; ++t) sum += (double)part[(size_t)t * kNParams];
    AdamStep ad;
    ad.p = B.params; ad.m = B.adam_m; ad.v = B.adam_v;
    ad.grad = B.grad ? B.grad + (size_t)s * kNParams : nullptr;
    ad.w1 = 1.0 - B.beta1; ad.w2 = 1.0 - B.beta2; ad.beta2 = B.beta2; ad.eps = B.eps_d;
    ad.bc2_sqrt = s_bc2_sqrt;
    ad.neg_step = s_neg_step;
    adam_update(ad, e, (float)sum);
}

// PRIO: block 0 of a learner leaves max(priority[0 .. size)) in *prio_max after a call that trained (a call below the size gate wrote no
// priority and leaves the maximum alone, and so does a learner marked bad: it has returned above).  fmaxf is exact: the order is free.
template <bool PRIO>
__global__ __launch_bounds__(kApplyBlock) void k_dwide_finish(const DWideArgs A)
{
    const int tid = threadIdx.x;
    const DWideBrain& B = A.b[blockIdx.y];
    const long long* hdr = work_hdr(B);
    if (hdr[kHdrBad]) return;   // (uniform) this learner's buffers stay exactly as they were
    if (blockIdx.x == 0 && tid == 0) {
        B.state[0] = hdr[kHdrSteps] + (hdr[kHdrTrain] ? A.n_steps : 0);
        B.state[1] = hdr[kHdrCalls] + 1;
    }
    const int e = blockIdx.x * kApplyBlock + tid;
    if (B.sync_target && e < kNParams) B.target[e] = B.params[e];   // D3QN.py:125-126, on the caller's schedule, also below the size gate
    if constexpr (PRIO) {
        __shared__ float prio_red[kApplyBlock];
        const long long size = hdr[kHdrSize];
        if (blockIdx.x != 0 || !hdr[kHdrTrain] || size <= 0) return;   // (uniform)
        const float* pr = A.p[blockIdx.y].priority;
        float mx = 0.0f;      // (priorities are |.|: never below zero)
        for (long long i = tid; i < size; i += kApplyBlock) mx = fmaxf(mx, pr[i]);
        prio_red[tid] = mx;
        __syncthreads();
        for (int o = kApplyBlock / 2; o > 0; o >>= 1) {
            if (tid < o) prio_red[tid] = fmaxf(prio_red[tid], prio_red[tid + o]);
            __syncthreads();
        }
        if (tid == 0) *A.p[blockIdx.y].prio_max = prio_red[0];
    }
}

}  // namespace

int rl_learn_dueling_wide_supported_impl(int kind) { return kind == RL_D3QN ? 1 : 0; }

size_t rl_learn_dueling_wide_work_bytes_impl(int batch)
{
    const size_t tiles = (size_t)(batch + kDRows - 1) / kDRows;
    return kHdrBytes + tiles * kNParams * sizeof(float) + dwide_sums_bytes((int)tiles) + tiles * kStashFloats * sizeof(float);
}

template <bool PRIO>
static int dwide_launch(const char* who, rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                        int n_steps, const int32_t* slots, void* const* work, hipStream_t stream)
{
    DWideArgs a{};
    const long long* bad[RL_MAX_CAPTURE_BRAINS];
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        DWideBrain& b = a.b[i];
        b.params = l.params; b.target = l.target; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.work = (char*)work[i];
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2);
        b.gamma = l.gamma; b.eps_d = learn_decimal(l.eps);
        b.min_size = l.min_size; b.sync_target = l.sync_target;
        if (PRIO) { a.p[i].priority = prios[i].priority; a.p[i].prio_max = prios[i].prio_max; }
        bad[i] = (const long long*)work[i] + kHdrBad;
    }
    a.slots = slots; a.err = h->err_flag; a.seed = h->cfg.seed; a.n_steps = n_steps;
    a.batch = learners[0].batch; a.tiles = (a.batch + kDRows - 1) / kDRows;
    {   // the large dynamic-LDS window (158 KB), per kernel: asked for at every call -- idempotent, host-only, and right on whatever device is current
        hipError_t e = hipFuncSetAttribute((const void*)k_dwide_forward, hipFuncAttributeMaxDynamicSharedMemorySize, kDLdsBytes);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_dwide_backward<PRIO>, hipFuncAttributeMaxDynamicSharedMemorySize, kDLdsBytes);
        if (e != hipSuccess) { rl_set_error("%s: hipFuncSetAttribute(%d bytes of LDS) failed: %s", who, kDLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    const int pblocks = (kNParams + kApplyBlock - 1) / kApplyBlock;
    hipLaunchKernelGGL(k_dwide_check, dim3(n_learners), dim3(kApplyBlock), 0, stream, a);
    for (int s = 0; s < n_steps; ++s) {
        a.step = s;
        hipLaunchKernelGGL(k_dwide_forward, dim3(a.tiles, n_learners), dim3(kDBlock), kDLdsBytes, stream, a);
        hipLaunchKernelGGL(k_dwide_backward<PRIO>, dim3(a.tiles, n_learners), dim3(kDBlock), kDLdsBytes, stream, a);
        hipLaunchKernelGGL(k_dwide_apply, dim3(pblocks, n_learners), dim3(kApplyBlock), 0, stream, a);
    }
    hipLaunchKernelGGL(k_dwide_finish<PRIO>, dim3(pblocks, n_learners), dim3(kApplyBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: kernel launch failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return rl_learn_wide_pack_launch(learners, n_learners, bad, stream);
}

int rl_learn_dueling_wide_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps,
                                 const int32_t* slots, void* const* work, hipStream_t stream)
{
    return dwide_launch<false>("rl_learn_dueling_wide", h, learners, rings, nullptr, n_learners, n_steps, slots, work, stream);
}

// rl_learn_prioritized_wide: the same launches with the <true> instantiations of the backward and finish kernels; the work buffer is
// rl_learn_dueling_wide's, byte for byte.
int rl_learn_prioritized_wide_supported_impl(int kind) { return kind == RL_PERD3QN ? 1 : 0; }

int rl_learn_prioritized_wide_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                                     int n_steps, const int32_t* slots, void* const* work, hipStream_t stream)
{
    return dwide_launch<true>("rl_learn_prioritized_wide", h, learners, rings, prios, n_learners, n_steps, slots, work, stream);
}
