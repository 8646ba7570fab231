// rl_learn_wide.hip -- the DQN brain's minibatch update (rl_learn.hip: k_learn_dqn) on WIDE minibatches: 1 .. RL_LEARN_WIDE_MAX rows, split
// into 32-row tiles that run side by side on otherwise idle CUs.  This build's own: the reference trains one world on 5 x 32 rows per
// train() (Models/DQN.py:80-83, 142-153); a run of hundreds of worlds appends a thousand times that per learning episode.
//
// Reference (paths under ReinLife/Models):
//   DQNAgent.train              DQN.py:80-83     the size gate (> 1000 transitions) and the hard target copy after EVERY train()
//   train(q, q_target, ...)     DQN.py:142-153   per step: sample, smooth-L1 of q[a] against r + gamma max q'(s') done_mask, Adam step
//   Qnet.forward                DQN.py:126-130   153 -> 128 -> 64 -> 8, ReLU between
//
// Shape.  A call queues 2 n_steps + 3 launches on the caller's stream; nothing is read back, no launch is cooperative, no workgroup
// waits for another.  Every learner has a work buffer: a 64-byte header | partial[T][n_params] | tile_loss[T], T = ceil(batch / 32).
//   k_wide_check   grid (n_learners), once.  Ring size and the gate size > min_size as k_learn_dqn computes them; every slot of a call
//                  that trains is range-checked (a bad one: error-flag code 6, first in table order); the header gets {trains, bad,
//                  steps taken, calls made, size} AS READ AT ENTRY.  Every later kernel reads these words and never a counter that a
//                  workgroup of its own launch writes; a learner marked bad is left alone by all of them.
//   k_wide_tile    grid (T, n_learners), per step s.  Tile t holds batch rows 32 t .. min(32 t + 31, batch - 1); rows beyond the batch are
//                  zero rows with a zero loss gradient.  k_learn_dqn's LDS layout and arithmetic, thread for thread: target forward, eval
//                  forward, smooth-L1, the backward pass through the two ReLUs -- with row_g scaled by 1.0f / batch of the WHOLE batch.
//                  Where k_learn_dqn hands a parameter's gradient (the f32 sum over the tile's rows, ascending) to Adam, the tile
//                  stores it to partial[t]; consecutive threads store consecutive floats.  Thread 0 stores the f32 sum of the rows' loss
//                  terms.  Parameters are only read here.
//   k_wide_apply   grid (ceil(n_params / 256), n_learners), per step s, one thread per parameter: g = (float)(sum_t (double)partial[t][i]),
//                  t ascending, then rl_learn_dev.h's adam_update with t_adam = steps at entry + s + 1.  The sum is double because T
//                  partials of mixed sign would otherwise add T - 1 float roundings to a gradient the tests hold to 1e-5 of its tensor's
//                  maximum; with one tile the round trip float -> double -> float is the identity, which is what makes batch <= 32 the
//                  bits of rl_learn.  lane l reads partial[t][e0 + l]: coalesced per tile.
//   k_wide_finish  grid (ceil(n_params / 256), n_learners), once: target <- params where sync_target is set (also below the gate);
//                  state[0] += steps made, state[1] += 1.
//   packing        rl_learn_merge.hip's k_pack_device (what rl_policy_pack_device launches), skipping a learner marked bad.
#include "rl_learn_dev.h"

int rl_learn_wide_pack_launch(const rl_learner*, int, const long long* const*, hipStream_t);   // rl_learn_merge.hip

namespace {

constexpr int kLearnBlock = 256;
constexpr int kLearnRows = 32;                 // rows of a tile
constexpr int kXS = 156, kH1S = 128, kH2S = 68;   // LDS row strides in floats (16-byte aligned rows; 153 / 128 / 64 used)
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
constexpr int kLearnSite = RL_SITE_LEARN;
// state-dict-flat offsets of the DQN network (fc1.w fc1.b fc2.w fc2.b fc3.w fc3.b)
constexpr int oW1 = 0, oB1 = 153 * 128, oW2 = oB1 + 128, oB2 = oW2 + 128 * 64, oW3 = oB2 + 64, oB3 = oW3 + 64 * 8, kNParams = oB3 + 8;
// the work buffer: header words (long long), then the partial rows, then the tile losses
constexpr int kHdrBytes = 64;
enum { kHdrTrain = 0, kHdrBad = 1, kHdrSteps = 2, kHdrCalls = 3, kHdrSize = 4 };

struct WideBrain {
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

struct WideArgs {
    WideBrain b[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;        // [n_learners][n_steps][batch] or null
    int32_t* err;
    uint64_t seed;
    int n_steps, batch, tiles;
    int step;                    // k_wide_tile, k_wide_apply: the step of this launch
};

__device__ inline long long* work_hdr(const WideBrain& B) { return (long long*)B.work; }
__device__ inline float* work_partial(const WideBrain& B) { return (float*)(B.work + kHdrBytes); }
__device__ inline float* work_tile_loss(const WideBrain& B, int tiles) { return work_partial(B) + (size_t)tiles * kNParams; }

constexpr int kWideLdsFloats = 2 * kLearnRows * kXS + 2 * kLearnRows * kH1S + 2 * kLearnRows * kH2S + kLearnRows * 8 + 5 * kLearnRows;
constexpr int kWideLdsBytes = kWideLdsFloats * 4 + 16;

__global__ __launch_bounds__(kLearnBlock) void k_wide_check(const WideArgs A)
{
    __shared__ int first_bad;
    const int tid = threadIdx.x, brain = blockIdx.x;
    const WideBrain& B = A.b[brain];
    const int batch = A.batch, n_steps = A.n_steps;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const bool train = size > B.min_size;
    int bad = 0x7fffffff;
    const int32_t* sl = A.slots ? A.slots + (size_t)brain * n_steps * batch : nullptr;
    if (sl && train) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        for (int i = tid; i < n_steps * batch; i += kLearnBlock)
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

// H[row][f] = (relu) (b[f] + sum_k W[f][k] X[row][k]), k ascending, for the 32 rows.  A thread owns feature f = tid % NOUT and
// RPT = NOUT / 8 consecutive rows; NINP = NIN rounded up to 4 (the rows' padding is zero, the weights beyond NIN are not read).
template <int NIN, int NOUT, int XS, int HS, bool RELU>
__device__ inline void wide_forward(const float* W, const float* bias, const float* X, float* H, int tid)
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

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending), stored to the tile's partial row.  A work item is (a chunk of 16
// outputs, one k): consecutive threads take consecutive k, so each of the 16 stores of a wave covers 256 contiguous bytes.
template <int NIN, int NOUT, int DS, int INS>
__device__ inline void wide_wgrad(float* out, const float* D, const float* IN, int tid)
{
    for (int item = tid; item < (NOUT / 16) * NIN; item += kLearnBlock) {
        const int oc = item / NIN, k = item - oc * NIN;
        float acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll 2
        for (int row = 0; row < kLearnRows; ++row) {
            const float x = IN[row * INS + k];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 d = *(const f32x4*)(D + row * DS + oc * 16 + 4 * q);
                acc[4 * q + 0] = fmaf(d.x, x, acc[4 * q + 0]); acc[4 * q + 1] = fmaf(d.y, x, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(d.z, x, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(d.w, x, acc[4 * q + 3]);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) out[(oc * 16 + i) * NIN + k] = acc[i];
    }
}
template <int NOUT, int DS>
__device__ inline void wide_bgrad(float* out, const float* D, int tid)
{
    if (tid < NOUT) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kLearnRows; ++row) g += D[row * DS + tid];
        out[tid] = g;
    }
}

__global__ __launch_bounds__(kLearnBlock) void k_wide_tile(const WideArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float wide_lds[];
    float* xs = wide_lds;                           // [32][156] state
    float* xp = xs + kLearnRows * kXS;              // [32][156] state_prime
    float* h1 = xp + kLearnRows * kXS;              // [32][128]
    float* d1 = h1 + kLearnRows * kH1S;             // [32][128]
    float* h2 = d1 + kLearnRows * kH1S;             // [32][68]
    float* d2 = h2 + kLearnRows * kH2S;             // [32][68]
    float* q = d2 + kLearnRows * kH2S;              // [32][8]
    float* row_g = q + kLearnRows * 8;              // [32] dLoss / dq[a]
    float* row_r = row_g + kLearnRows;              // [32] reward
    float* row_mask = row_r + kLearnRows;           // [32] 1 - done
    float* row_loss = row_mask + kLearnRows;        // [32] smooth-L1 term (reused as max q')
    int* row_a = (int*)(row_loss + kLearnRows);     // [32] action
    __shared__ int row_slot[kLearnRows];

    const int tid = threadIdx.x, tile = blockIdx.x, brain = blockIdx.y;
    const WideBrain& B = A.b[brain];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform) below the gate, or a bad slot: nothing of this learner is written
    const int batch = A.batch, n_steps = A.n_steps, s = A.step;
    const long long size = hdr[kHdrSize], calls = hdr[kHdrCalls];
    const int j = tile * kLearnRows + tid;         // (tid < 32) this thread's row of the batch
    const float inv_batch = 1.0f / (float)batch;
    float* part = work_partial(B) + (size_t)tile * kNParams;

    // ---- the tile's rows: rows >= batch are zero rows with a zero loss gradient ----
    if (tid < kLearnRows) {
        const bool in = j < batch;
        int slot = 0;
        if (in) {
            if (A.slots) slot = A.slots[((size_t)brain * n_steps + s) * batch + j];
            else slot = (int)(((uint64_t)rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)calls, (uint32_t)kLearnSite, (uint32_t)(s * batch + j)).x * (uint64_t)size) >> 32);
        }
        row_slot[tid] = in ? slot : -1;
        row_a[tid] = in ? (int)B.r_action[slot] & 7 : 0;
        row_r[tid] = in ? B.r_reward[slot] : 0.0f;
        row_mask[tid] = in ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kLearnRows * kXS; i += kLearnBlock) {
        const int row = i / kXS, k = i - row * kXS, slot = row_slot[row];
        const bool live = slot >= 0 && k < RL_OBS_DIM;
        xs[i] = live ? B.r_state[(size_t)slot * RL_OBS_DIM + k] : 0.0f;
        xp[i] = live ? B.r_state_prime[(size_t)slot * RL_OBS_DIM + k] : 0.0f;
    }
    __syncthreads();
    // ---- max_a Q_target(s') ----
    wide_forward<153, 128, kXS, kH1S, true>(B.target + oW1, B.target + oB1, xp, h1, tid);
    __syncthreads();
    wide_forward<128, 64, kH1S, kH2S, true>(B.target + oW2, B.target + oB2, h1, h2, tid);
    __syncthreads();
    wide_forward<64, 8, kH2S, 8, false>(B.target + oW3, B.target + oB3, h2, q, tid);
    __syncthreads();
    if (tid < kLearnRows) {
        float mx = q[tid * 8];
        for (int a = 1; a < 8; ++a) mx = fmaxf(mx, q[tid * 8 + a]);
        row_loss[tid] = mx;
    }
    __syncthreads();
    // ---- Q_eval(s) ----
    wide_forward<153, 128, kXS, kH1S, true>(B.params + oW1, B.params + oB1, xs, h1, tid);
    __syncthreads();
    wide_forward<128, 64, kH1S, kH2S, true>(B.params + oW2, B.params + oB2, h1, h2, tid);
    __syncthreads();
    wide_forward<64, 8, kH2S, 8, false>(B.params + oW3, B.params + oB3, h2, q, tid);
    __syncthreads();
    // ---- smooth-L1 (beta = 1) of q[a] against r + gamma max q' done_mask, and its gradient ----
    if (tid < kLearnRows) {
        const float target = row_r[tid] + (B.gamma * row_loss[tid]) * row_mask[tid];
        const float td = q[tid * 8 + row_a[tid]] - target, ad = fabsf(td);
        const bool in = j < batch;
        row_loss[tid] = in ? (ad < 1.0f ? (0.5f * td) * td : ad - 0.5f) : 0.0f;
        row_g[tid] = in ? fminf(fmaxf(td, -1.0f), 1.0f) * inv_batch : 0.0f;
    }
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        for (int r = 0; r < kLearnRows; ++r) sum += row_loss[r];
        work_tile_loss(B, A.tiles)[tile] = sum;
    }
    // ---- backward through the two ReLUs ----
    for (int i = tid; i < kLearnRows * 64; i += kLearnBlock) {
        const int row = i >> 6, o = i & 63;
        d2[row * kH2S + o] = h2[row * kH2S + o] > 0.0f ? B.params[oW3 + row_a[row] * 64 + o] * row_g[row] : 0.0f;
    }
    __syncthreads();
    {
        const int k = tid & 127, row0 = (tid >> 7) * 16;
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 2
        for (int o = 0; o < 64; o += 4) {
            float w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = B.params[oW2 + (o + i) * 128 + k];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f32x4 d = *(const f32x4*)(d2 + (row0 + r) * kH2S + o);
                acc[r] = fmaf(w[0], d.x, acc[r]); acc[r] = fmaf(w[1], d.y, acc[r]);
                acc[r] = fmaf(w[2], d.z, acc[r]); acc[r] = fmaf(w[3], d.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) d1[(row0 + r) * kH1S + k] = h1[(row0 + r) * kH1S + k] > 0.0f ? acc[r] : 0.0f;
    }
    __syncthreads();
    // ---- the tile's partial gradient, parameter by parameter ----
    wide_wgrad<153, 128, kH1S, kXS>(part + oW1, d1, xs, tid);
    wide_bgrad<128, kH1S>(part + oB1, d1, tid);
    wide_wgrad<128, 64, kH2S, kH1S>(part + oW2, d2, h1, tid);
    wide_bgrad<64, kH2S>(part + oB2, d2, tid);
    for (int item = tid; item < 8 * 64; item += kLearnBlock) {   // fc3: only the taken action's row of a minibatch row is non-zero
        const int a = item >> 6, k = item & 63;
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kLearnRows; ++row) g = fmaf(row_a[row] == a ? row_g[row] : 0.0f, h2[row * kH2S + k], g);
        part[oW3 + item] = g;
    }
    if (tid < 8) {
        float g = 0.0f;
        for (int row = 0; row < kLearnRows; ++row) g += row_a[row] == tid ? row_g[row] : 0.0f;
        part[oB3 + tid] = g;
    }
}

__global__ __launch_bounds__(kLearnBlock) void k_wide_apply(const WideArgs A)
{
    __shared__ double s_bc2_sqrt, s_neg_step;
    const int tid = threadIdx.x;
    const WideBrain& B = A.b[blockIdx.y];
    const long long* hdr = work_hdr(B);
    if (!hdr[kHdrTrain] || hdr[kHdrBad]) return;   // (uniform)
    const int s = A.step, tiles = A.tiles;
    if (tid == 0) {
        const double t = (double)(hdr[kHdrSteps] + s + 1);
        s_bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
        s_neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
    }
    __syncthreads();
    const float inv_batch = 1.0f / (float)A.batch;
    if (blockIdx.x == 0 && tid == 0 && B.loss) {
        const float* tl = work_tile_loss(B, tiles);
        double sum = 0.0;
        for (int t = 0; t < tiles; ++t) sum += (double)tl[t];
        B.loss[s] = (float)sum * inv_batch;
    }
    const int e = blockIdx.x * kLearnBlock + tid;
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

__global__ __launch_bounds__(kLearnBlock) void k_wide_finish(const WideArgs A)
{
    const int tid = threadIdx.x;
    const WideBrain& B = A.b[blockIdx.y];
    const long long* hdr = work_hdr(B);
    if (hdr[kHdrBad]) return;   // (uniform) this learner's buffers stay exactly as they were
    if (blockIdx.x == 0 && tid == 0) {
        B.state[0] = hdr[kHdrSteps] + (hdr[kHdrTrain] ? A.n_steps : 0);
        B.state[1] = hdr[kHdrCalls] + 1;
    }
    const int e = blockIdx.x * kLearnBlock + tid;
    if (B.sync_target && e < kNParams) B.target[e] = B.params[e];   // DQN.py:83: after every train(), also below the size gate
}

}  // namespace

int rl_learn_wide_supported_impl(int kind) { return kind == RL_DQN ? 1 : 0; }

size_t rl_learn_wide_work_bytes_impl(int batch)
{
    const size_t tiles = (size_t)(batch + kLearnRows - 1) / kLearnRows;
    return kHdrBytes + tiles * kNParams * sizeof(float) + ((tiles * sizeof(float) + 15) & ~(size_t)15);
}

int rl_learn_wide_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
                         void* const* work, hipStream_t stream)
{
    WideArgs a{};
    const long long* bad[RL_MAX_CAPTURE_BRAINS];
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        WideBrain& b = a.b[i];
        b.params = l.params; b.target = l.target; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.work = (char*)work[i];
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2);
        b.gamma = l.gamma; b.eps_d = learn_decimal(l.eps);
        b.min_size = l.min_size; b.sync_target = l.sync_target;
        bad[i] = (const long long*)work[i] + kHdrBad;
    }
    a.slots = slots; a.err = h->err_flag; a.seed = h->cfg.seed; a.n_steps = n_steps;
    a.batch = learners[0].batch; a.tiles = (a.batch + kLearnRows - 1) / kLearnRows;
    {   // the large dynamic-LDS window (92 KB): asked for at every call -- idempotent, host-only, and right on whatever device is current
        const hipError_t e = hipFuncSetAttribute((const void*)k_wide_tile, hipFuncAttributeMaxDynamicSharedMemorySize, kWideLdsBytes);
        if (e != hipSuccess) { rl_set_error("rl_learn_wide: hipFuncSetAttribute(%d bytes of LDS) failed: %s", kWideLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    const int pblocks = (kNParams + kLearnBlock - 1) / kLearnBlock;
    hipLaunchKernelGGL(k_wide_check, dim3(n_learners), dim3(kLearnBlock), 0, stream, a);
    for (int s = 0; s < n_steps; ++s) {
        a.step = s;
        hipLaunchKernelGGL(k_wide_tile, dim3(a.tiles, n_learners), dim3(kLearnBlock), kWideLdsBytes, stream, a);
        hipLaunchKernelGGL(k_wide_apply, dim3(pblocks, n_learners), dim3(kLearnBlock), 0, stream, a);
    }
    hipLaunchKernelGGL(k_wide_finish, dim3(pblocks, n_learners), dim3(kLearnBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_wide: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return rl_learn_wide_pack_launch(learners, n_learners, bad, stream);
}
