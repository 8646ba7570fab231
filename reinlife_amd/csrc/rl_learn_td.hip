// rl_learn_td.hip -- k_learn_perdqn: the PERDQN brain's minibatch updates on the device (rl_learn_td), from the replay rings
// rl_capture_transitions fills to the packed weights the acting kernels read, with no host round trip.  The memory's draw
// (rl_learn_td_draw) is rl_learn_prio.hip's, instantiated for this memory.
//
// Reference (ReinLife/Models/PERDQN.py):
//   DQN.forward                 :311-325  fc.0 153 -> 64, fc.2 64 -> 64, fc.4 64 -> 8, ReLU between: 14,536 parameters
//   PERDQNAgent.train_model     the update below; torch.optim.Adam with default betas and eps
//   PERDQNAgent.learn           update_target_model() after EVERY trigger, also when nothing trained (rl_learner.sync_target)
//   Memory / SumTree            the prioritised memory: e = 0.01, a = 0.6, beta 0.4 -> 1 by 0.001 per sample()
// Three things the reference does are reproduced as they are, not repaired (the project's rule: rl_learn_dueling.hip on PERD3QN):
//   1. append_sample's error is |old_val - target[0][action]| with old_val a VIEW of the tensor the line before overwrote: exactly 0.
//      Every stored row gets (0 + e) ** a as a float32 torch scalar (rl_tdprio.p_new, made by the caller with torch), whatever the row.
//   2. train_model's loss is (FloatTensor(is_weights) * F.mse_loss(pred, target)).mean() with mse_loss already the scalar mean:
//      loss = mean(w) * mean((pred - target)^2), and dloss / dpred_i = mean(w) * 2 (pred_i - target_i) / B.  No per-row weighting.
//   3. is_weight_i = (n_entries * p_i / total) ** -beta divided by its maximum over the batch: total and n_entries cancel, this is
//      (p_i / min_j p_j) ** -beta over the batch rows -- no sum tree and no total are needed.  beta = min(1, beta + increment) in
//      double at every sample(), by repeated addition.
// pred_i = Q(s_i)[a_i] and target_i = r_i + (1 - done_i) gamma max_a Q_target(s'_i), both from the step's pre-update parameters; after
// the forward passes every batch row's priority becomes (|pred_i - target_i| + e) ** a in float32.
//
// Shape.  One 512-thread workgroup per learning brain makes the call's n_steps updates one after the other; workgroups never meet.
// Plain f32 FMA, every sum by ONE thread in a fixed order (k ascending, rows ascending), no float atomics, no gradient buffer unless the
// caller gives one.  Same buffers, same bits, whatever else is in the launch.
//
// LDS (112,128 bytes dynamic of the workgroup's 163,840; one workgroup per CU is all a brain ever has), 64 minibatch rows:
//   X   [64][156]  s' for the target forward (which keeps only max q'), then s for the eval forward and fc.0's weight gradient
//   H1  [64][68], H2 [64][68]   relu(fc.0), relu(fc.2) of the network being evaluated
//   D1  [64][68], D2 [64][68]   the back-propagated rows
//   Q   [64][8], the per-row scalars, the packer's scales
// The weights are NOT staged in LDS: a thread of a forward pass owns one output feature and eight rows, so a weight is read from
// global memory by 8 threads of 8 different waves and multiplied 8 times by each -- 58 KB of parameters that stay in the CU's L1 / L2
// for the whole call (one workgroup per CU, nothing else competes).  Staging them would save 7 of 8 cache reads per weight at the cost of
// an LDS write and an LDS read each, and X + H + D + the network (170 KB) does not fit beside each other anyway: it would take the
// tiling of rl_learn_dueling.hip.  That was the decision from the code.  MEASURED since: a step takes 107 us, far above
// its arithmetic, and the first suspect is exactly these reads -- a lane per feature means 64 distinct cache lines per load instruction
// in the forward passes, as in k_learn_dqn.  Weight tiles through LDS, read coalesced, are the next thing to try; not done here.
// All of D1 / D2 is complete before the first parameter changes (fc.2 and fc.4 are inputs of the backward pass).
//
// Packing.  After the last step the workgroup rewrites `packed` from the final parameters: rl_policy.hip's pack_in_layer 153 -> 64,
// pack_hidden_layer 64 -> 64 and pack_head 64 -> 8 at layout_of(RL_PERDQN), split to the NEAREST f16 (split2_host with rne: PERDQN's
// alone among the kinds), bit for bit.
#include "rl_learn_dev.h"

#include <math.h>

namespace {

constexpr int kTBlock = 512;
constexpr int kTRows = 64;                     // rows of a minibatch at most (rl_learner.batch)
constexpr int kTXS = 156, kTHS = 68;           // LDS row strides in floats (16-byte aligned rows; 153 / 64 used, the padding of X is zero)
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
// state-dict-flat offsets of the PERDQN network (fc.0.w fc.0.b fc.2.w fc.2.b fc.4.w fc.4.b)
constexpr int oW1 = 0, oB1 = 153 * 64, oW2 = oB1 + 64, oB2 = oW2 + 64 * 64, oW3 = oB2 + 64, oB3 = oW3 + 64 * 8, kNParams = oB3 + 8;
static_assert(kNParams == 14536, "the PERDQN network has 14,536 parameters");
constexpr int kNFeat = 64 + 64 + 8;            // output features of the three layers (the packer's scales)

struct TdBrain {
    float *params, *target, *adam_m, *adam_v;
    long long* state;
    float* packed;
    float* loss;
    float* grad;
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const unsigned long long* r_count;
    long long r_capacity;
    double lr, beta1, beta2, eps_d;   // the decimal values the caller's floats stand for (learn_decimal)
    float gamma;
    int batch, min_size, sync_target;
    float* priority;                  // [ring capacity]
    double* beta;                     // [1]
    double beta_increment;
    float prio_e, prio_a;
    float* is_weight;                 // [n_steps][batch] or null
};

struct TdArgs {
    TdBrain b[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;             // [n_learners][n_steps][batch]
    int32_t* err;
    int n_steps;
};

constexpr int kTLdsFloats = kTRows * kTXS + 4 * kTRows * kTHS + kTRows * 8 + 6 * kTRows + 2 * kNFeat;
constexpr int kTLdsBytes = kTLdsFloats * 4;
static_assert(kTLdsBytes + 1024 <= 160 * 1024, "k_learn_perdqn's LDS map must fit a workgroup's 160 KiB");

// H[row][f] = (relu) (b[f] + sum_k W[f][k] X[row][k]), k ascending, for the 64 rows.  A thread owns feature f = tid % NOUT and
// RPT = NOUT / 8 consecutive rows (the rows' padding is zero, the weights beyond NIN are not read).
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

// Q [64][8] of the network P on the rows in X (H1, H2 as the file's header says).  Ends with a barrier.
__device__ __forceinline__ void td_network(const float* P, const float* X, float* h1, float* h2, float* q, int tid)
{
    td_forward<153, 64, kTXS, kTHS, true>(P + oW1, P + oB1, X, h1, tid);
    __syncthreads();
    td_forward<64, 64, kTHS, kTHS, true>(P + oW2, P + oB2, h1, h2, tid);
    __syncthreads();
    td_forward<64, 8, kTHS, 8, false>(P + oW3, P + oB3, h2, q, tid);
    __syncthreads();
}

// the minibatch's rows of `src` (state or state_prime of the ring) -> X [64][156]; rows without a slot and columns >= 153 are zero
// (issuing a thread's 20 loads ahead of its stores was tried and measured: 132.0 against 132.8 us per call, so the step is not bound here)
__device__ __forceinline__ void td_stage_rows(const float* src, const int* row_slot, float* X, int tid)
{
    for (int i = tid; i < kTRows * kTXS; i += kTBlock) {
        const int row = i / kTXS, k = i - row * kTXS, slot = row_slot[row];
        X[i] = (slot >= 0 && k < RL_OBS_DIM) ? src[(size_t)slot * RL_OBS_DIM + k] : 0.0f;
    }
}

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending) and Adam at once.  A work item is (a chunk of 8 outputs, one k):
// consecutive threads take consecutive k, so the parameter traffic of a chunk row is contiguous.
template <int NIN, int NOUT, int DS, int INS>
__device__ __forceinline__ void td_wgrad(const AdamStep& a, int off, const float* D, const float* IN, int tid)
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
        for (int i = 0; i < 8; ++i) adam_update(a, off + (oc * 8 + i) * NIN + k, acc[i]);
    }
}
__device__ __forceinline__ void td_bgrad(const AdamStep& a, int off, const float* D, int tid)
{
    if (tid < 64) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kTRows; ++row) g += D[row * kTHS + tid];
        adam_update(a, off + tid, g);
    }
}

// rl_policy_pack_weights(RL_PERDQN, P) -> packed, by the whole workgroup.  sc / un: LDS [kNFeat] each (features of fc.0, fc.2, fc.4).
__device__ __forceinline__ void td_pack(const float* P, float* packed, float* sc, float* un, int tid)
{
    const Layout L = layout_of(RL_PERDQN);
    if (tid < kNFeat) {   // feature_scales: 2^(kScaleExp - exponent(max |W[o][:]|))
        const int n_in = tid < 64 ? 153 : 64;
        const float* w = tid < 64 ? P + oW1 + tid * 153 : tid < 128 ? P + oW2 + (tid - 64) * 64 : P + oW3 + (tid - 128) * 64;
        float mx = 0.0f;
#pragma unroll 4
        for (int k = 0; k < n_in; ++k) mx = fmaxf(mx, fabsf(w[k]));
        row_scale(mx, sc[tid], un[tid]);
    }
    __syncthreads();
    uint4* d1 = (uint4*)(packed + L.l1);
    for (int u = tid; u < kInChunks * 2 * 64; u += kTBlock) {        // pack_in_layer 153 -> 64: [c][t][plane][lane]
        const int lane = u & 63, t = (u >> 6) & 1, c = u >> 7;
        const int o = 32 * t + (lane & 31), k0 = 16 * c + 8 * (lane >> 5);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = k0 + e < 153 ? P[oW1 + o * 153 + k0 + e] * sc[o] : 0.0f;
        uint4* dst = d1 + ((c * 2 + t) * kPlanes) * 64 + lane;
        learn_store_fragment_rne(x, dst, dst + 64);
    }
    uint4* d2 = (uint4*)(packed + L.l2a);
    for (int u = tid; u < 4 * 2 * 64; u += kTBlock) {                // pack_hidden_layer 64 -> 64: [s = 2t + c][t2][plane][lane]
        const int lane = u & 63, t2 = (u >> 6) & 1, s = u >> 7;
        const int o = 32 * t2 + (lane & 31);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = P[oW2 + o * 64 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[64 + o];
        uint4* dst = d2 + ((s * 2 + t2) * kPlanes) * 64 + lane;
        learn_store_fragment_rne(x, dst, dst + 64);
    }
    uint4* d3 = (uint4*)(packed + L.ha);
    for (int u = tid; u < 4 * 64; u += kTBlock) {                    // pack_head 64 -> 8: [2t + c][plane][lane], rows >= 8 zero
        const int lane = u & 63, s = u >> 6;
        const int o = lane & 31;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = o < 8 ? P[oW3 + o * 64 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[128 + o] : 0.0f;
        uint4* dst = d3 + (s * kPlanes) * 64 + lane;
        learn_store_fragment_rne(x, dst, dst + 64);
    }
    // write_epilogue_consts: per output tile t2 and lane half h [unscale 16 | bias 16], feature 32 t2 + (r&3) + 8(r>>2) + 4h
    for (int i = tid; i < 128 + 128; i += kTBlock) {
        const int second = i >= 128, ii = second ? i - 128 : i;
        const int r = ii & 15, th = ii >> 5;
        const int o = 32 * (th >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (th & 1);
        const float val = (ii & 16) ? P[(second ? oB2 : oB1) + o] : un[(second ? 64 : 0) + o];
        packed[(second ? L.l2a + frag_floats(4, 2) : L.l1 + frag_floats(kInChunks, 2)) + ii] = val;
    }
    if (tid < 16) packed[L.ha + head_consts_off(2) + tid] = tid < 8 ? un[128 + tid] : P[oB3 + tid - 8];
}

__global__ __launch_bounds__(kTBlock) void k_learn_perdqn(const TdArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float td_lds[];
    float* xs = td_lds;                             // X  [64][156]
    float* h1 = xs + kTRows * kTXS;                 // H1 [64][68]
    float* h2 = h1 + kTRows * kTHS;                 // H2 [64][68]
    float* d1 = h2 + kTRows * kTHS;                 // D1 [64][68]
    float* d2 = d1 + kTRows * kTHS;                 // D2 [64][68]
    float* q = d2 + kTRows * kTHS;                  // [64][8]
    float* row_g = q + kTRows * 8;                  // [64] dloss / dpred
    float* row_r = row_g + kTRows;                  // [64] reward
    float* row_mask = row_r + kTRows;               // [64] 1 - done
    float* row_y = row_mask + kTRows;               // [64] max q', then (pred - target)^2
    float* row_w = row_y + kTRows;                  // [64] is_weight
    float* row_p = row_w + kTRows;                  // [64] the row's priority as it stands at this step
    float* sc = row_p + kTRows;                     // [kNFeat] the packer's feature scales
    float* un = sc + kNFeat;
    __shared__ int first_bad;
    __shared__ int row_slot[kTRows];
    __shared__ int row_a[kTRows];
    __shared__ float mean_w;

    const int tid = threadIdx.x, brain = blockIdx.x;
    const TdBrain& B = A.b[brain];
    const int batch = B.batch, n_steps = A.n_steps;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const long long calls = B.state[1];
    long long steps_taken = B.state[0];
    const bool train = size > B.min_size;

    if (train) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        const int32_t* sl = A.slots + (size_t)brain * n_steps * batch;
        for (int i = tid; i < n_steps * batch; i += kTBlock)
            if (sl[i] < 0 || sl[i] >= size) atomicMin(&first_bad, i);
        __syncthreads();
        const int bad = first_bad;
        if (bad != 0x7fffffff) {
            if (tid == 0 && A.err && atomicCAS(A.err, 0, kErrLearnSlot) == 0) { A.err[1] = brain; A.err[2] = bad / batch; A.err[3] = sl[bad]; }
            return;   // (uniform) this brain's buffers stay exactly as they were
        }
    }
    const float inv_batch = 1.0f / (float)batch;
    double beta = train ? *B.beta : 0.0;
    for (int s = 0; train && s < n_steps; ++s) {
        // The buffers' addresses are re-read as opaque values in every step, as in k_learn_d3qn: otherwise the compiler hoists the
        // per-lane addresses of the step's parameter accesses in front of this loop and spills them.
        typedef float __attribute__((address_space(1))) gf;
        gf *gP = (gf*)B.params, *gT = (gf*)B.target, *gAM = (gf*)B.adam_m, *gAV = (gf*)B.adam_v, *gGR = (gf*)B.grad;
        asm volatile("" : "+s"(gP), "+s"(gT), "+s"(gAM), "+s"(gAV), "+s"(gGR));
        float *P = (float*)gP, *T = (float*)gT, *AM = (float*)gAM, *AV = (float*)gAV, *GR = (float*)gGR;
        beta = fmin(1.0, beta + B.beta_increment);   // Memory.sample: before the weights are made
        // ---- the minibatch: rows >= batch are zero rows with a zero loss gradient ----
        if (tid < kTRows) {
            const bool in = tid < batch;
            const int slot = in ? A.slots[((size_t)brain * n_steps + s) * batch + tid] : 0;
            row_slot[tid] = in ? slot : -1;
            row_a[tid] = in ? (int)B.r_action[slot] & 7 : 0;
            row_r[tid] = in ? B.r_reward[slot] : 0.0f;
            row_mask[tid] = in ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
            row_p[tid] = in ? B.priority[slot] : 0.0f;
        }
        __syncthreads();
        // ---- is_weight_i = (p_i / min_j p_j) ** -beta, and its mean (rows ascending) ----
        if (tid < kTRows) {
            float p_min = row_p[0];
            for (int j = 1; j < batch; ++j) p_min = fminf(p_min, row_p[j]);
            const float w = tid < batch ? (float)pow((double)row_p[tid] / (double)p_min, -beta) : 0.0f;
            row_w[tid] = w;
            if (B.is_weight && tid < batch) B.is_weight[(size_t)s * batch + tid] = w;
        }
        td_stage_rows(B.r_state_prime, row_slot, xs, tid);
        __syncthreads();
        if (tid == 0) {
            float sum = 0.0f;
            for (int j = 0; j < batch; ++j) sum += row_w[j];
            mean_w = sum * inv_batch;
        }
        // ---- max_a Q_target(s') ----
        td_network(T, xs, h1, h2, q, tid);
        if (tid < kTRows) {
            float mx = q[tid * 8];
            for (int a = 1; a < 8; ++a) mx = fmaxf(mx, q[tid * 8 + a]);
            row_y[tid] = mx;
        }
        td_stage_rows(B.r_state, row_slot, xs, tid);   // (the target forward is done with X)
        __syncthreads();
        // ---- Q(s), the loss mean(w) * mean((pred - target)^2), dloss / dpred and the rows' new priorities ----
        td_network(P, xs, h1, h2, q, tid);
        if (tid < kTRows) {
            const float target = row_r[tid] + row_mask[tid] * (B.gamma * row_y[tid]);
            const float td = q[tid * 8 + row_a[tid]] - target;
            const bool in = tid < batch;
            if (in) B.priority[row_slot[tid]] = powf(fabsf(td) + B.prio_e, B.prio_a);   // duplicated slots: equal rows, equal bits
            row_y[tid] = in ? td * td : 0.0f;
            row_g[tid] = in ? mean_w * ((2.0f * td) * inv_batch) : 0.0f;
        }
        __syncthreads();
        if (tid == 0 && B.loss) {
            float sum = 0.0f;
            for (int j = 0; j < batch; ++j) sum += row_y[j];
            B.loss[s] = mean_w * (sum * inv_batch);
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
        // ---- gradients and Adam, parameter by parameter (nothing below reads a parameter of this network) ----
        const double t = (double)(steps_taken + 1);
        AdamStep ad;
        ad.p = P; ad.m = AM; ad.v = AV;
        ad.grad = GR ? GR + (size_t)s * kNParams : nullptr;
        ad.w1 = 1.0 - B.beta1; ad.w2 = 1.0 - B.beta2; ad.beta2 = B.beta2; ad.eps = B.eps_d;
        ad.bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
        ad.neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
        td_wgrad<153, 64, kTHS, kTXS>(ad, oW1, d1, xs, tid);
        td_bgrad(ad, oB1, d1, tid);
        td_wgrad<64, 64, kTHS, kTHS>(ad, oW2, d2, h1, tid);
        td_bgrad(ad, oB2, d2, tid);
        {   // fc.4: only the taken action's row of a minibatch row is non-zero
            const int a = tid >> 6, k = tid & 63;
            float g = 0.0f;
#pragma unroll 4
            for (int row = 0; row < kTRows; ++row) g = fmaf(row_a[row] == a ? row_g[row] : 0.0f, h2[row * kTHS + k], g);
            adam_update(ad, oW3 + tid, g);
        }
        if (tid < 8) {
            float g = 0.0f;
            for (int row = 0; row < kTRows; ++row) g += row_a[row] == tid ? row_g[row] : 0.0f;
            adam_update(ad, oB3 + tid, g);
        }
        ++steps_taken;
        __syncthreads();   // the next step (and the packer) read the new parameters and priorities
    }
    if (B.sync_target)     // PERDQNAgent.learn: update_target_model() after every trigger, also below the size gate
        for (int i = tid; i < kNParams; i += kTBlock) B.target[i] = B.params[i];
    if (tid == 0) {
        B.state[0] = steps_taken; B.state[1] = calls + 1;
        if (train) *B.beta = beta;
    }
    td_pack(B.params, B.packed, sc, un, tid);
}

// ---- rl_learn_td_stamp: THIS BUILD'S OWN -- the TD-error priority of the rows appended since the last draw --------------------------
// PERDQN.py:113-128 (append_sample) spells out (|Q(s)[a] - (r + (1 - done) gamma max_a Q_target(s'))| + e) ** a for a row it stores and
// computes (0 + e) ** a (quirk 1 above).  k_td_stamp computes what the code spells out, for the draws' window -- the slots of
// [*seen, *count) mod capacity, all rows once count - seen >= capacity -- and k_td_stamp_seen, the launch behind it, closes the window
// (*seen = *count), so that a following draw, unchanged code, stamps nothing.
//
// One 512-thread workgroup per (learner, 64 window rows): the steps of k_learn_perdqn between its row scalars and its priority write,
// made by the SAME functions (td_stage_rows, td_network) on the same LDS map without D1 / D2 -- a stamped priority is, bit for bit,
// what k_learn_perdqn writes for that row from the same parameters.  77,568 bytes of dynamic LDS: two workgroups share a CU.  The
// weights come from L1 / L2 by td_forward's strided reads, as in the learner (DESIGN.md 5.29 on what that costs here).
// Reads seen and count, writes priority[slot] of window rows and nothing else; no atomics; no workgroup waits for another.
struct StampBrain {
    const float *params, *target;
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const unsigned long long* r_count;
    long long r_capacity;
    float* priority;
    unsigned long long* seen;
    float gamma, prio_e, prio_a;
};
struct StampArgs {
    StampBrain b[RL_MAX_CAPTURE_BRAINS];
};

constexpr int kSLdsFloats = kTRows * kTXS + 2 * kTRows * kTHS + kTRows * 8 + 3 * kTRows;
constexpr int kSLdsBytes = kSLdsFloats * 4;
static_assert(2 * (kSLdsBytes + 1024) <= 160 * 1024, "two k_td_stamp workgroups must fit a CU's 160 KiB");

__global__ __launch_bounds__(kTBlock) void k_td_stamp(const StampArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float td_lds[];
    float* xs = td_lds;                             // X  [64][156]
    float* h1 = xs + kTRows * kTXS;                 // H1 [64][68]
    float* h2 = h1 + kTRows * kTHS;                 // H2 [64][68]
    float* q = h2 + kTRows * kTHS;                  // [64][8]
    float* row_r = q + kTRows * 8;                  // [64] reward
    float* row_mask = row_r + kTRows;               // [64] 1 - done
    float* row_y = row_mask + kTRows;               // [64] max q'
    __shared__ int row_slot[kTRows];
    __shared__ int row_a[kTRows];

    const int tid = threadIdx.x;
    const StampBrain& B = A.b[blockIdx.y];
    const unsigned long long count = *B.r_count, seen = *B.seen, cap = (unsigned long long)B.r_capacity;
    const unsigned long long size = count < cap ? count : cap;
    const unsigned long long fresh = count > seen ? count - seen : 0ull;   // rows appended since the last draw (k_prio_prepare's rule)
    const bool all = fresh >= cap;
    const unsigned long long n_window = all ? size : fresh;
    const unsigned long long j0 = (unsigned long long)blockIdx.x * kTRows;
    if (j0 >= n_window) return;                     // (uniform) beyond the window

    if (tid < kTRows) {   // window row j sits in slot j (the whole ring) or (seen + j) mod capacity: always < size <= capacity
        const unsigned long long j = j0 + tid;
        const bool in = j < n_window;
        const int slot = in ? (int)(all ? j : (seen % cap + j) % cap) : 0;
        row_slot[tid] = in ? slot : -1;
        row_a[tid] = in ? (int)B.r_action[slot] & 7 : 0;
        row_r[tid] = in ? B.r_reward[slot] : 0.0f;
        row_mask[tid] = in ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
    }
    __syncthreads();
    td_stage_rows(B.r_state_prime, row_slot, xs, tid);
    __syncthreads();
    // ---- max_a Q_target(s') ----
    td_network(B.target, xs, h1, h2, q, tid);
    if (tid < kTRows) {
        float mx = q[tid * 8];
        for (int a = 1; a < 8; ++a) mx = fmaxf(mx, q[tid * 8 + a]);
        row_y[tid] = mx;
    }
    td_stage_rows(B.r_state, row_slot, xs, tid);    // (the target forward is done with X)
    __syncthreads();
    // ---- Q(s) and the rows' priorities: k_learn_perdqn's expressions ----
    td_network(B.params, xs, h1, h2, q, tid);
    if (tid < kTRows && row_slot[tid] >= 0) {
        const float target = row_r[tid] + row_mask[tid] * (B.gamma * row_y[tid]);
        const float td = q[tid * 8 + row_a[tid]] - target;
        B.priority[row_slot[tid]] = powf(fabsf(td) + B.prio_e, B.prio_a);
    }
}

// the launch behind k_td_stamp, its only reader of `seen`: one thread per learner
__global__ __launch_bounds__(64) void k_td_stamp_seen(const StampArgs A, int n_learners)
{
    const int i = threadIdx.x;
    if (i < n_learners) *A.b[i].seen = *A.b[i].r_count;
}

}  // namespace

int rl_learn_td_stamp_launch(rl_world*, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, hipStream_t stream)
{
    StampArgs a{};
    long long max_cap = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        StampBrain& b = a.b[i];
        b.params = l.params; b.target = l.target;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.priority = tds[i].priority; b.seen = tds[i].seen;
        b.gamma = l.gamma; b.prio_e = tds[i].prio_e; b.prio_a = tds[i].prio_a;
        max_cap = r.capacity > max_cap ? r.capacity : max_cap;
    }
    {   // 76 KB of dynamic LDS: asked for at every call, as rl_learn_td does
        const hipError_t e = hipFuncSetAttribute((const void*)k_td_stamp, hipFuncAttributeMaxDynamicSharedMemorySize, kSLdsBytes);
        if (e != hipSuccess) { rl_set_error("rl_learn_td_stamp: hipFuncSetAttribute(%d bytes of LDS) failed: %s", kSLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    hipLaunchKernelGGL(k_td_stamp, dim3((unsigned)((max_cap + kTRows - 1) / kTRows), n_learners), dim3(kTBlock), kSLdsBytes, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_td_stamp: launch of the stamp kernel failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    hipLaunchKernelGGL(k_td_stamp_seen, dim3(1), dim3(64), 0, stream, a, n_learners);
    e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_td_stamp: launch of the window kernel failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

int rl_learn_td_supported_impl(int kind) { return kind == RL_PERDQN ? 1 : 0; }

int rl_learn_td_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                       const int32_t* slots, hipStream_t stream)
{
    TdArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        const rl_tdprio& p = tds[i];
        TdBrain& b = a.b[i];
        b.params = l.params; b.target = l.target; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.packed = l.packed; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2);
        b.gamma = l.gamma; b.eps_d = learn_decimal(l.eps);
        b.batch = l.batch; b.min_size = l.min_size; b.sync_target = l.sync_target;
        b.priority = p.priority; b.beta = p.beta; b.beta_increment = p.beta_increment; b.prio_e = p.prio_e; b.prio_a = p.prio_a;
        b.is_weight = p.is_weight;
    }
    a.slots = slots; a.err = h->err_flag; a.n_steps = n_steps;
    {   // the large dynamic-LDS window (110 KB): asked for at every call -- idempotent, host-only, and right on whatever device is current
        const hipError_t e = hipFuncSetAttribute((const void*)k_learn_perdqn, hipFuncAttributeMaxDynamicSharedMemorySize, kTLdsBytes);
        if (e != hipSuccess) { rl_set_error("rl_learn_td: hipFuncSetAttribute(%d bytes of LDS) failed: %s", kTLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    hipLaunchKernelGGL(k_learn_perdqn, dim3(n_learners), dim3(kTBlock), kTLdsBytes, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_td: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}
