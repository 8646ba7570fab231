// rl_learn_td_wide.hip -- the PERDQN brain's minibatch update (rl_learn_td.hip: k_learn_perdqn) on WIDE minibatches: 1 .. RL_LEARN_TD_WIDE_MAX
// rows, split into 64-row tiles that run side by side on otherwise idle CUs.  This build's own: the reference trains one world on ONE
// minibatch of 64 per train_model() (PERDQN.py:130-186); a run of hundreds of worlds appends more rows per learning episode than the
// 20,000-row memory holds.
//
// Reference (ReinLife/Models/PERDQN.py):
//   DQN.forward                 :311-325  fc.0 153 -> 64, fc.2 64 -> 64, fc.4 64 -> 8, ReLU between: 14,536 parameters
//   PERDQNAgent.train_model     :130-186  the update; loss = mean(is_w) * mean((pred - target)^2) (rl_learn_td.hip, quirk 2)
//   Memory.sample               is_w_i = (p_i / min_j p_j) ** -beta over the WHOLE batch (quirk 3); beta = min(1, beta + increment) in double
//
// What makes this learner unlike the other wide ones: the rows of a step meet in TWO scalars, p_min (needed before any row's weight
// exists) and mean(is_w) (a factor of every row's loss gradient), and the tiles of a step rewrite the very priorities those scalars are
// read from.  So the scalars are made by a launch of their own, in front of the step's tiles: no workgroup reads a priority that a
// workgroup of the same launch can write.
//
// Shape.  A call queues 3 n_steps + 3 launches (RL_LEARN_TD_WIDE_LAUNCHES) on the caller's stream; nothing is read back, no launch is
// cooperative, no workgroup waits for another, no float atomics.  Every learner has a work buffer: a 64-byte header | partial[T][14,536] |
// tile_sq[T], T = ceil(batch / 64).
//   k_tdw_check    grid (n_learners), once.  rl_learn_wide.hip's k_wide_check: ring size, the gate size > min_size, every slot of a call
//                  that trains range-checked (a bad one: error-flag code 6, first in table order); the header gets {trains, bad, steps
//                  taken, calls made, size} AS READ AT ENTRY, and beta as it stands.  A learner marked bad is left alone by every later
//                  kernel: none of its buffers is written, priorities and beta included.
//   k_tdw_weights  grid (n_learners), per step s.  beta = min(1, beta + beta_increment) in double (kept in the header from step to
//                  step); the step's B priorities as they stand; p_min by fminf, rows ascending within a tile (one thread per tile),
//                  then the tiles ascending -- fminf is associative, so this is the fold over all rows ascending; w_i =
//                  (float)pow((double)p_i / (double)p_min, -beta), each by its own thread; per tile the f32 sum of w, rows ascending; the
//                  tile sums added in double in tile order from -0.0 (the additive identity) and rounded to float ONCE; mean_w = that *
//                  (1.0f / B) into the header; w into is_weight[s] when given.
//   k_tdw_tile     grid (T, n_learners), per step s.  Tile t holds batch rows 64 t .. min(64 t + 63, B - 1); rows beyond the batch are zero
//                  rows with a zero loss gradient.  k_learn_perdqn's LDS map and arithmetic, thread for thread: the target forward on s',
//                  the eval forward on s (td_forward's chain from the bias, k ascending), td = pred - target, row_g = mean_w * ((2 td) *
//                  (1 / B)) with B the WHOLE batch, priority[slot] = powf(fabsf(td) + prio_e, prio_a) by the row's own tile (duplicated
//                  slots, also across tiles, are equal rows and carry equal bits: no winner rule), the backward pass through the two
//                  ReLUs.  Where k_learn_perdqn hands a parameter's gradient (the f32 sum over the tile's rows, ascending) to Adam, the
//                  tile stores it to partial[t]; thread 0 stores the f32 sum of the rows' td^2.  Parameters are only read here.
//   k_tdw_apply    grid (ceil(14,536 / 256), n_learners), per step s, one thread per parameter: g = (float)(sum_t (double)partial[t][i]),
//                  t ascending from -0.0, then rl_learn_dev.h's adam_update with t_adam = steps at entry + s + 1.  loss[s] = mean_w *
//                  (sum_sq * (1 / B)), sum_sq from the tile sums as mean_w's sum.  With one tile float -> double -> float is the
//                  identity: batch <= 64 gives the bits of rl_learn_td.
//   k_tdw_finish   grid (ceil(14,536 / 256), n_learners), once: target <- params where sync_target is set (also below the gate);
//                  state[0] += steps made, state[1] += 1; *beta <- the header's iff the learner trained.
//   packing        rl_learn_merge.hip's k_pack_device for RL_PERDQN (split to the nearest f16), skipping a learner marked bad.
//
// LDS of a tile (112,640 bytes dynamic): X [64][156], H1 H2 D1 D2 [64][68], Q [64][8], four row scalars [64] -- one workgroup per CU.
// The weights come from L1 / L2 by td_forward's strided reads, as in rl_learn_td.hip (its header on what that costs).
#include "rl_learn_dev.h"

#include <math.h>

int rl_learn_wide_pack_launch(const rl_learner*, int, const long long* const*, hipStream_t);   // rl_learn_merge.hip

namespace {

constexpr int kTBlock = 512;
constexpr int kTRows = 64;                     // rows of a tile
constexpr int kTXS = 156, kTHS = 68;           // LDS row strides in floats (16-byte aligned rows; 153 / 64 used, the padding of X is zero)
constexpr int kABlock = 256;                   // k_tdw_apply, k_tdw_finish
constexpr int kMaxBatch = RL_LEARN_TD_WIDE_MAX;
constexpr int kMaxTiles = kMaxBatch / kTRows;
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
// state-dict-flat offsets of the PERDQN network (fc.0.w fc.0.b fc.2.w fc.2.b fc.4.w fc.4.b)
constexpr int oW1 = 0, oB1 = 153 * 64, oW2 = oB1 + 64, oB2 = oW2 + 64 * 64, oW3 = oB2 + 64, oB3 = oW3 + 64 * 8, kNParams = oB3 + 8;
static_assert(kNParams == 14536, "the PERDQN network has 14,536 parameters");
static_assert(kMaxBatch % kTRows == 0 && kMaxTiles <= kTBlock, "one thread per tile in k_tdw_weights");
// the work buffer: header words (8 bytes each), then the partial rows, then the tiles' sums of td^2
constexpr int kHdrBytes = 64;
enum { kHdrTrain = 0, kHdrBad = 1, kHdrSteps = 2, kHdrCalls = 3, kHdrSize = 4, kHdrBeta = 5 /* a double */, kHdrMeanW = 6 /* a float */ };

struct TdwBrain {
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
    float* priority;                  // [ring capacity]
    double* beta;                     // [1]
    double beta_increment;
    float prio_e, prio_a;
    float* is_weight;                 // [n_steps][batch] or null
};

struct TdwArgs {
    TdwBrain b[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;             // [n_learners][n_steps][batch]
    int32_t* err;
    int n_steps, batch, tiles;
    int step;                         // k_tdw_weights, k_tdw_tile, k_tdw_apply: the step of this launch
};
static_assert(sizeof(TdwArgs) <= 4096, "kernel arguments are passed by value");

__device__ inline long long* work_hdr(const TdwBrain& B) { return (long long*)B.work; }
__device__ inline double* work_beta(const TdwBrain& B) { return (double*)(B.work + 8 * kHdrBeta); }
__device__ inline float* work_mean_w(const TdwBrain& B) { return (float*)(B.work + 8 * kHdrMeanW); }
__device__ inline float* work_partial(const TdwBrain& B) { return (float*)(B.work + kHdrBytes); }
__device__ inline float* work_tile_sq(const TdwBrain& B, int tiles) { return work_partial(B) + (size_t)tiles * kNParams; }

constexpr int kTLdsFloats = kTRows * kTXS + 4 * kTRows * kTHS + kTRows * 8 + 4 * kTRows;
constexpr int kTLdsBytes = kTLdsFloats * 4;
static_assert(kTLdsBytes + 1024 <= 160 * 1024, "k_tdw_tile's LDS map must fit a workgroup's 160 KiB");

__global__ __launch_bounds__(kABlock) void k_tdw_check(const TdwArgs A)
{
    __shared__ int first_bad;
    const int tid = threadIdx.x, brain = blockIdx.x;
    const TdwBrain& B = A.b[brain];
    const int batch = A.batch, n_steps = A.n_steps;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const bool train = size > B.min_size;
    int bad = 0x7fffffff;
    const int32_t* sl = A.slots + (size_t)brain * n_steps * batch;
    if (train) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        for (long long i = tid; i < (long long)n_steps * batch; i += kABlock)
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
        *work_beta(B) = *B.beta;
        hdr[kHdrMeanW] = hdr[7] = 0;
    }
}

// row j of the batch sits at j + j / 64 in the weights pass' LDS columns: a thread per tile walks its 64 rows without bank conflicts
__device__ inline int wrow(int j) { return j + (j >> 6); }

__global__ __launch_bounds__(kTBlock) void k_tdw_weights(const TdwArgs A)
{
    __shared__ float row_p[kMaxBatch + kMaxTiles];   // the rows' priorities as they stand at this step
    __shared__ float row_w[kMaxBatch + kMaxTiles];   // is_weight
    __shared__ float tile_min[kMaxTiles], tile_sum[kMaxTiles];
    const int tid = threadIdx.x, brain = blockIdx.x;
    const TdwBrain& B = A.b[brain];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform) below the gate, or a bad slot: nothing of this learner is written
    const int batch = A.batch, tiles = A.tiles, s = A.step;
    const double beta = fmin(1.0, *work_beta(B) + B.beta_increment);   // Memory.sample: before the weights are made
    const int32_t* sl = A.slots + ((size_t)brain * A.n_steps + s) * batch;
    for (int j = tid; j < batch; j += kTBlock) row_p[wrow(j)] = B.priority[sl[j]];
    __syncthreads();
    if (tid < tiles) {
        const int j0 = tid * kTRows, j1 = j0 + kTRows < batch ? j0 + kTRows : batch;
        float m = row_p[wrow(j0)];
        for (int j = j0 + 1; j < j1; ++j) m = fminf(m, row_p[wrow(j)]);
        tile_min[tid] = m;
    }
    __syncthreads();
    float p_min = tile_min[0];
    for (int t = 1; t < tiles; ++t) p_min = fminf(p_min, tile_min[t]);
    for (int j = tid; j < batch; j += kTBlock) {
        const float w = (float)pow((double)row_p[wrow(j)] / (double)p_min, -beta);
        row_w[wrow(j)] = w;
        if (B.is_weight) B.is_weight[(size_t)s * batch + j] = w;
    }
    __syncthreads();
    if (tid < tiles) {
        const int j0 = tid * kTRows, j1 = j0 + kTRows < batch ? j0 + kTRows : batch;
        float sum = 0.0f;
        for (int j = j0; j < j1; ++j) sum += row_w[wrow(j)];
        tile_sum[tid] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = -0.0;   // the additive identity: one tile gives its f32 sum back, bit for bit
        for (int t = 0; t < tiles; ++t) sum += (double)tile_sum[t];
        *work_mean_w(B) = (float)sum * (1.0f / (float)batch);
        *work_beta(B) = beta;   // (this workgroup is the header's only reader and writer in this launch)
    }
}

// H[row][f] = (relu) (b[f] + sum_k W[f][k] X[row][k]), k ascending, for the 64 rows.  A thread owns feature f = tid % NOUT and
// RPT = NOUT / 8 consecutive rows (the rows' padding is zero, the weights beyond NIN are not read).  rl_learn_td.hip's td_forward.
template <int NIN, int NOUT, int XS, int HS, bool RELU>
__device__ __forceinline__ void td_forward(const float* W, const float* bias, const float* X, float* H, int tid)
{
    constexpr int RPT = NOUT / 8;
    const int f = tid % NOUT, row0 = (tid / NOUT) * RPT;
    const float* w = W + f * NIN;
    float acc[RPT];
    const float b = bias[f];
#pragma unroll
    for (int r = 0; r < RPT; ++r) acc[r] = b;
#pragma unroll 2
    for (int k = 0; k < NIN; k += 4) {
        float wk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wk[i] = (k + i < NIN) ? w[k + i] : 0.0f;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const f32x4 x = *(const f32x4*)(X + (row0 + r) * XS + k);
            acc[r] = fmaf(wk[0], x.x, acc[r]); acc[r] = fmaf(wk[1], x.y, acc[r]);
            acc[r] = fmaf(wk[2], x.z, acc[r]); acc[r] = fmaf(wk[3], x.w, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) H[(row0 + r) * HS + f] = RELU ? fmaxf(acc[r], 0.0f) : acc[r];
}

// Q [64][8] of the network P on the rows in X.  Ends with a barrier.
__device__ __forceinline__ void td_network(const float* P, const float* X, float* h1, float* h2, float* q, int tid)
{
    td_forward<153, 64, kTXS, kTHS, true>(P + oW1, P + oB1, X, h1, tid);
    __syncthreads();
    td_forward<64, 64, kTHS, kTHS, true>(P + oW2, P + oB2, h1, h2, tid);
    __syncthreads();
    td_forward<64, 8, kTHS, 8, false>(P + oW3, P + oB3, h2, q, tid);
    __syncthreads();
}

// the tile's rows of `src` (state or state_prime of the ring) -> X [64][156]; rows without a slot and columns >= 153 are zero
__device__ __forceinline__ void td_stage_rows(const float* src, const int* row_slot, float* X, int tid)
{
    for (int i = tid; i < kTRows * kTXS; i += kTBlock) {
        const int row = i / kTXS, k = i - row * kTXS, slot = row_slot[row];
        X[i] = (slot >= 0 && k < RL_OBS_DIM) ? src[(size_t)slot * RL_OBS_DIM + k] : 0.0f;
    }
}

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending), stored to the tile's partial row: rl_learn_td.hip's td_wgrad with the
// store in Adam's place.  A work item is (a chunk of 8 outputs, one k): consecutive threads store consecutive floats.
template <int NIN, int NOUT, int DS, int INS>
__device__ __forceinline__ void tdw_wgrad(float* out, const float* D, const float* IN, int tid)
{
    for (int item = tid; item < (NOUT / 8) * NIN; item += kTBlock) {
        const int oc = item / NIN, k = item - oc * NIN;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kTRows; ++row) {
            const float x = IN[row * INS + k];
            const f32x4 d0 = *(const f32x4*)(D + row * DS + oc * 8), d1 = *(const f32x4*)(D + row * DS + oc * 8 + 4);
            acc[0] = fmaf(d0.x, x, acc[0]); acc[1] = fmaf(d0.y, x, acc[1]); acc[2] = fmaf(d0.z, x, acc[2]); acc[3] = fmaf(d0.w, x, acc[3]);
            acc[4] = fmaf(d1.x, x, acc[4]); acc[5] = fmaf(d1.y, x, acc[5]); acc[6] = fmaf(d1.z, x, acc[6]); acc[7] = fmaf(d1.w, x, acc[7]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) out[(oc * 8 + i) * NIN + k] = acc[i];
    }
}
__device__ __forceinline__ void tdw_bgrad(float* out, const float* D, int tid)
{
    if (tid < 64) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kTRows; ++row) g += D[row * kTHS + tid];
        out[tid] = g;
    }
}

__global__ __launch_bounds__(kTBlock) void k_tdw_tile(const TdwArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float tdw_lds[];
    float* xs = tdw_lds;                            // X  [64][156]
    float* h1 = xs + kTRows * kTXS;                 // H1 [64][68]
    float* h2 = h1 + kTRows * kTHS;                 // H2 [64][68]
    float* d1 = h2 + kTRows * kTHS;                 // D1 [64][68]
    float* d2 = d1 + kTRows * kTHS;                 // D2 [64][68]
    float* q = d2 + kTRows * kTHS;                  // [64][8]
    float* row_g = q + kTRows * 8;                  // [64] dloss / dpred
    float* row_r = row_g + kTRows;                  // [64] reward
    float* row_mask = row_r + kTRows;               // [64] 1 - done
    float* row_y = row_mask + kTRows;               // [64] max q', then (pred - target)^2
    __shared__ int row_slot[kTRows];
    __shared__ int row_a[kTRows];

    const int tid = threadIdx.x, tile = blockIdx.x, brain = blockIdx.y;
    const TdwBrain& B = A.b[brain];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform) below the gate, or a bad slot: nothing of this learner is written
    const int batch = A.batch, s = A.step;
    const int j = tile * kTRows + tid;             // (tid < 64) this thread's row of the batch
    const int tile_rows = batch - tile * kTRows < kTRows ? batch - tile * kTRows : kTRows;
    const float inv_batch = 1.0f / (float)batch;
    const float mean_w = *work_mean_w(B);
    const float *P = B.params, *T = B.target;
    float* part = work_partial(B) + (size_t)tile * kNParams;

    // ---- the tile's rows: rows >= batch are zero rows with a zero loss gradient ----
    if (tid < kTRows) {
        const bool in = j < batch;
        const int slot = in ? A.slots[((size_t)brain * A.n_steps + s) * batch + j] : 0;
        row_slot[tid] = in ? slot : -1;
        row_a[tid] = in ? (int)B.r_action[slot] & 7 : 0;
        row_r[tid] = in ? B.r_reward[slot] : 0.0f;
        row_mask[tid] = in ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
    }
    __syncthreads();
    td_stage_rows(B.r_state_prime, row_slot, xs, tid);
    __syncthreads();
    // ---- max_a Q_target(s') ----
    td_network(T, xs, h1, h2, q, tid);
    if (tid < kTRows) {
        float mx = q[tid * 8];
        for (int a = 1; a < 8; ++a) mx = fmaxf(mx, q[tid * 8 + a]);
        row_y[tid] = mx;
    }
    td_stage_rows(B.r_state, row_slot, xs, tid);   // (the target forward is done with X)
    __syncthreads();
    // ---- Q(s), dloss / dpred with the whole batch's mean(w) and 1 / B, and the rows' new priorities ----
    td_network(P, xs, h1, h2, q, tid);
    if (tid < kTRows) {
        const float target = row_r[tid] + row_mask[tid] * (B.gamma * row_y[tid]);
        const float td = q[tid * 8 + row_a[tid]] - target;
        const bool in = j < batch;
        if (in) B.priority[row_slot[tid]] = powf(fabsf(td) + B.prio_e, B.prio_a);   // duplicated slots, also in other tiles: equal rows, equal bits
        row_y[tid] = in ? td * td : 0.0f;
        row_g[tid] = in ? mean_w * ((2.0f * td) * inv_batch) : 0.0f;
    }
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        for (int r = 0; r < tile_rows; ++r) sum += row_y[r];
        work_tile_sq(B, A.tiles)[tile] = sum;
    }
    // ---- backward through the two ReLUs ----
    for (int i = tid; i < kTRows * 64; i += kTBlock) {
        const int row = i >> 6, o = i & 63;
        d2[row * kTHS + o] = h2[row * kTHS + o] > 0.0f ? P[oW3 + row_a[row] * 64 + o] * row_g[row] : 0.0f;
    }
    __syncthreads();
    {
        const int k = tid & 63, row0 = (tid >> 6) * 8;
        float acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.0f;
#pragma unroll 2
        for (int o = 0; o < 64; o += 4) {
            float w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = P[oW2 + (o + i) * 64 + k];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const f32x4 d = *(const f32x4*)(d2 + (row0 + r) * kTHS + o);
                acc[r] = fmaf(w[0], d.x, acc[r]); acc[r] = fmaf(w[1], d.y, acc[r]);
                acc[r] = fmaf(w[2], d.z, acc[r]); acc[r] = fmaf(w[3], d.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) d1[(row0 + r) * kTHS + k] = h1[(row0 + r) * kTHS + k] > 0.0f ? acc[r] : 0.0f;
    }
    __syncthreads();
    // ---- the tile's partial gradient, parameter by parameter ----
    tdw_wgrad<153, 64, kTHS, kTXS>(part + oW1, d1, xs, tid);
    tdw_bgrad(part + oB1, d1, tid);
    tdw_wgrad<64, 64, kTHS, kTHS>(part + oW2, d2, h1, tid);
    tdw_bgrad(part + oB2, d2, tid);
    {   // fc.4: only the taken action's row of a minibatch row is non-zero
        const int a = tid >> 6, k = tid & 63;
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kTRows; ++row) g = fmaf(row_a[row] == a ? row_g[row] : 0.0f, h2[row * kTHS + k], g);
        part[oW3 + tid] = g;
    }
    if (tid < 8) {
        float g = 0.0f;
        for (int row = 0; row < kTRows; ++row) g += row_a[row] == tid ? row_g[row] : 0.0f;
        part[oB3 + tid] = g;
    }
}

__global__ __launch_bounds__(kABlock) void k_tdw_apply(const TdwArgs A)
{
    __shared__ double s_bc2_sqrt, s_neg_step;
    const int tid = threadIdx.x;
    const TdwBrain& B = A.b[blockIdx.y];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform)
    const int s = A.step, tiles = A.tiles;
    if (tid == 0) {
        const double t = (double)(hdr[kHdrSteps] + s + 1);
        s_bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
        s_neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0 && B.loss) {
        const float* sq = work_tile_sq(B, tiles);
        const float inv_batch = 1.0f / (float)A.batch;
        double sum = -0.0;
        for (int t = 0; t < tiles; ++t) sum += (double)sq[t];
        B.loss[s] = *work_mean_w(B) * ((float)sum * inv_batch);
    }
    const int e = blockIdx.x * kABlock + tid;
    if (e >= kNParams) return;
    const float* part = work_partial(B) + e;
    double sum = -0.0;
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

__global__ __launch_bounds__(kABlock) void k_tdw_finish(const TdwArgs A)
{
    const int tid = threadIdx.x;
    const TdwBrain& B = A.b[blockIdx.y];
    const long long* hdr = work_hdr(B);
    if (hdr[kHdrBad]) return;   // (uniform) this learner's buffers stay exactly as they were
    if (blockIdx.x == 0 && tid == 0) {
        B.state[0] = hdr[kHdrSteps] + (hdr[kHdrTrain] ? A.n_steps : 0);
        B.state[1] = hdr[kHdrCalls] + 1;
        if (hdr[kHdrTrain]) *B.beta = *work_beta(B);
    }
    const int e = blockIdx.x * kABlock + tid;
    if (B.sync_target && e < kNParams) B.target[e] = B.params[e];   // PERDQNAgent.learn: after every trigger, also below the size gate
}

}  // namespace

int rl_learn_td_wide_supported_impl(int kind) { return kind == RL_PERDQN ? 1 : 0; }

size_t rl_learn_td_wide_work_bytes_impl(int batch)
{
    const size_t tiles = (size_t)(batch + kTRows - 1) / kTRows;
    return kHdrBytes + tiles * kNParams * sizeof(float) + ((tiles * sizeof(float) + 15) & ~(size_t)15);
}

int rl_learn_td_wide_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                            const int32_t* slots, void* const* work, hipStream_t stream)
{
    TdwArgs a{};
    const long long* bad[RL_MAX_CAPTURE_BRAINS];
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        const rl_tdprio& p = tds[i];
        TdwBrain& b = a.b[i];
        b.params = l.params; b.target = l.target; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.work = (char*)work[i];
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2);
        b.gamma = l.gamma; b.eps_d = learn_decimal(l.eps);
        b.min_size = l.min_size; b.sync_target = l.sync_target;
        b.priority = p.priority; b.beta = p.beta; b.beta_increment = p.beta_increment; b.prio_e = p.prio_e; b.prio_a = p.prio_a;
        b.is_weight = p.is_weight;
        bad[i] = (const long long*)work[i] + kHdrBad;
    }
    a.slots = slots; a.err = h->err_flag; a.n_steps = n_steps;
    a.batch = learners[0].batch; a.tiles = (a.batch + kTRows - 1) / kTRows;
    {   // the large dynamic-LDS window (110 KB): asked for at every call -- idempotent, host-only, and right on whatever device is current
        const hipError_t e = hipFuncSetAttribute((const void*)k_tdw_tile, hipFuncAttributeMaxDynamicSharedMemorySize, kTLdsBytes);
        if (e != hipSuccess) { rl_set_error("rl_learn_td_wide: hipFuncSetAttribute(%d bytes of LDS) failed: %s", kTLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    const int pblocks = (kNParams + kABlock - 1) / kABlock;
    hipLaunchKernelGGL(k_tdw_check, dim3(n_learners), dim3(kABlock), 0, stream, a);
    for (int s = 0; s < n_steps; ++s) {
        a.step = s;
        hipLaunchKernelGGL(k_tdw_weights, dim3(n_learners), dim3(kTBlock), 0, stream, a);
        hipLaunchKernelGGL(k_tdw_tile, dim3(a.tiles, n_learners), dim3(kTBlock), kTLdsBytes, stream, a);
        hipLaunchKernelGGL(k_tdw_apply, dim3(pblocks, n_learners), dim3(kABlock), 0, stream, a);
    }
    hipLaunchKernelGGL(k_tdw_finish, dim3(pblocks, n_learners), dim3(kABlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_td_wide: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return rl_learn_wide_pack_launch(learners, n_learners, bad, stream);
}
