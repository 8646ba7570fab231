// rl_learn.hip -- k_learn_dqn: the DQN brain's minibatch updates on the device, from the replay rings rl_run_ex / rl_capture_transitions
// fill to the packed weights the acting kernels read, with no host round trip.
//
// Reference (paths under ReinLife/Models):
//   DQNAgent.train              DQN.py:80-83     the size gate (> 1000 transitions) and the hard target copy after EVERY train()
//   train(q, q_target, ...)     DQN.py:142-153   5 x (sample 32, smooth-L1 of q[a] against r + gamma max q'(s') done_mask, Adam step)
//   Qnet.forward                DQN.py:126-130   153 -> 128 -> 64 -> 8, ReLU between
//   torch.optim.Adam            betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad (DQN.py:52)
//
// Shape.  One 256-thread workgroup per learning brain makes the call's n_steps updates one after the other; workgroups never meet.
// Arithmetic is plain f32 FMA (v_fma_f32), every sum in a fixed order by ONE thread: a minibatch is 32 rows, so the matrix pipe's
// 32x32 tiles would run a quarter full on the weight gradients' K = 32, and the project's 2 x f16 split needs row maxima and
// re-splitting of activations AND gradients per step (docs/experiments.md, "rl_learn").  Same inputs, same bits, whatever else is in
// the launch.
//   LDS     the batch's observation rows x and x' [32][156], the hidden activations h1 [32][128] and h2 [32][68] (of the target network
//           first, then of the eval network), the back-propagated rows d1 [32][128], d2 [32][68], the Q rows and the per-row scalars
//   global  parameters, target, Adam moments (f32, state-dict-flat): weights are read through L1 / L2, and each parameter is updated by
//           the thread that summed its gradient
//   forward   a thread owns one output feature and a group of rows: the activations are LDS broadcasts (16 bytes per read)
//   backward  d2 = relu'(h2) * W3[a] * dq;  d1 = relu'(h1) * (W2^T d2);  then per parameter g = sum_rows d[row][out] * in[row][k] and
//             Adam at once -- no gradient buffer exists unless the caller asks for one (rl_learner.grad).  All of d1 / d2 is complete
//             before the first parameter changes (W2 and W3 are inputs of the backward pass).
//   packing   after the last step the workgroup rewrites `packed` from the final parameters: a port of rl_policy.hip's pack_in_layer /
//             pack_hidden_layer / pack_head / write_epilogue_consts for the toward-zero split, bit for bit (integer code, one multiply
//             by a power of two, one exact subtraction).
#include "rl_learn_dev.h"

namespace {

constexpr int kLearnBlock = 256;
constexpr int kLearnRows = 32;                 // rows of a minibatch at most (rl_learner.batch)
constexpr int kXS = 156, kH1S = 128, kH2S = 68;   // LDS row strides in floats (16-byte aligned rows; 153 / 128 / 64 used)
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
constexpr int kLearnSite = RL_SITE_LEARN;
// state-dict-flat offsets of the DQN network (fc1.w fc1.b fc2.w fc2.b fc3.w fc3.b)
constexpr int oW1 = 0, oB1 = 153 * 128, oW2 = oB1 + 128, oB2 = oW2 + 128 * 64, oW3 = oB2 + 64, oB3 = oW3 + 64 * 8, kNParams = oB3 + 8;

struct LearnBrain {
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
};

struct LearnArgs {
    LearnBrain b[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;        // [n_learners][n_steps][batch] or null
    int32_t* err;
    uint64_t seed;
    int n_steps;
};

constexpr int kLearnLdsFloats = 2 * kLearnRows * kXS + 2 * kLearnRows * kH1S + 2 * kLearnRows * kH2S + kLearnRows * 8 + 5 * kLearnRows + 2 * 200;
constexpr int kLearnLdsBytes = kLearnLdsFloats * 4 + 16;

// H[row][f] = (relu) (b[f] + sum_k W[f][k] X[row][k]), k ascending, for the 32 rows.  A thread owns feature f = tid % NOUT and
// RPT = NOUT / 8 consecutive rows; NINP = NIN rounded up to 4 (the rows' padding is zero, the weights beyond NIN are not read).
template <int NIN, int NOUT, int XS, int HS, bool RELU>
__device__ inline void learn_forward(const float* W, const float* bias, const float* X, float* H, int tid)
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

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending) and Adam at once.  A work item is (a chunk of 16 outputs, one k):
// consecutive threads take consecutive k, so the parameter traffic of a chunk row is contiguous.
template <int NIN, int NOUT, int DS, int INS>
__device__ inline void learn_wgrad(const AdamStep& a, int off, const float* D, const float* IN, int tid)
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
        for (int i = 0; i < 16; ++i) adam_update(a, off + (oc * 16 + i) * NIN + k, acc[i]);
    }
}
template <int NOUT, int DS>
__device__ inline void learn_bgrad(const AdamStep& a, int off, const float* D, int tid)
{
    if (tid < NOUT) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kLearnRows; ++row) g += D[row * DS + tid];
        adam_update(a, off + tid, g);
    }
}

// rl_policy_pack_weights(RL_DQN, P) -> packed, by the whole workgroup.  sc / un: LDS [200] each (features of fc1, fc2, fc3).
__device__ inline void learn_pack_dqn(const float* P, float* packed, float* sc, float* un, int tid)
{
    const Layout L = layout_of(RL_DQN);
    if (tid < 200) {   // feature_scales: 2^(kScaleExp - exponent(max |W[o][:]|))
        const int n_in = tid < 128 ? 153 : tid < 192 ? 128 : 64;
        const float* w = tid < 128 ? P + oW1 + tid * 153 : tid < 192 ? P + oW2 + (tid - 128) * 128 : P + oW3 + (tid - 192) * 64;
        float mx = 0.0f;
#pragma unroll 4
        for (int k = 0; k < n_in; ++k) mx = fmaxf(mx, fabsf(w[k]));
        row_scale(mx, sc[tid], un[tid]);
    }
    __syncthreads();
    uint4* d1 = (uint4*)(packed + L.l1);
    for (int u = tid; u < kInChunks * 4 * 64; u += kLearnBlock) {   // pack_in_layer: [c][t][plane][lane]
        const int lane = u & 63, t = (u >> 6) & 3, c = u >> 8;
        const int o = 32 * t + (lane & 31), k0 = 16 * c + 8 * (lane >> 5);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = k0 + e < 153 ? P[oW1 + o * 153 + k0 + e] * sc[o] : 0.0f;
        uint4* dst = d1 + ((c * 4 + t) * kPlanes) * 64 + lane;
        learn_store_fragment(x, dst, dst + 64);
    }
    uint4* d2 = (uint4*)(packed + L.l2a);
    for (int u = tid; u < 8 * 2 * 64; u += kLearnBlock) {            // pack_hidden_layer: [s = 2t + c][t2][plane][lane]
        const int lane = u & 63, t2 = (u >> 6) & 1, s = u >> 7;
        const int o = 32 * t2 + (lane & 31);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = P[oW2 + o * 128 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[128 + o];
        uint4* dst = d2 + ((s * 2 + t2) * kPlanes) * 64 + lane;
        learn_store_fragment(x, dst, dst + 64);
    }
    uint4* d3 = (uint4*)(packed + L.ha);
    for (int u = tid; u < 4 * 64; u += kLearnBlock) {                // pack_head: [2t + c][plane][lane], rows >= 8 zero
        const int lane = u & 63, s = u >> 6;
        const int o = lane & 31;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = o < 8 ? P[oW3 + o * 64 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[192 + o] : 0.0f;
        uint4* dst = d3 + (s * kPlanes) * 64 + lane;
        learn_store_fragment(x, dst, dst + 64);
    }
    // write_epilogue_consts: per output tile t2 and lane half h [unscale 16 | bias 16], feature 32 t2 + (r&3) + 8(r>>2) + 4h
    for (int i = tid; i < 256 + 128; i += kLearnBlock) {
        const int second = i >= 256, ii = second ? i - 256 : i;
        const int r = ii & 15, th = ii >> 5;
        const int o = 32 * (th >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (th & 1);
        const float val = (ii & 16) ? P[(second ? oB2 : oB1) + o] : un[(second ? 128 : 0) + o];
        packed[(second ? L.l2a + frag_floats(8, 2) : L.l1 + frag_floats(kInChunks, 4)) + ii] = val;
    }
    if (tid < 16) packed[L.ha + head_consts_off(2) + tid] = tid < 8 ? un[192 + tid] : P[oB3 + tid - 8];
}

__global__ __launch_bounds__(kLearnBlock) void k_learn_dqn(const LearnArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float learn_lds[];
    float* xs = learn_lds;                          // [32][156] state
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
    float* sc = (float*)(row_a + kLearnRows);       // [200] the packer's feature scales
    float* un = sc + 200;
    __shared__ int first_bad;
    __shared__ int row_slot[kLearnRows];

    const int tid = threadIdx.x, brain = blockIdx.x;
    const LearnBrain& B = A.b[brain];
    const int batch = B.batch, n_steps = A.n_steps;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const long long calls = B.state[1];
    long long steps_taken = B.state[0];

    if (A.slots && size > B.min_size) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        const int32_t* sl = A.slots + (size_t)brain * n_steps * batch;
        for (int i = tid; i < n_steps * batch; i += kLearnBlock)
            if (sl[i] < 0 || sl[i] >= size) atomicMin(&first_bad, i);
        __syncthreads();
        const int bad = first_bad;
        if (bad != 0x7fffffff) {
            if (tid == 0 && A.err && atomicCAS(A.err, 0, kErrLearnSlot) == 0) { A.err[1] = brain; A.err[2] = bad / batch; A.err[3] = sl[bad]; }
            return;   // (uniform) this brain's buffers stay exactly as they were
        }
    }
    const bool train = size > B.min_size;
    const float inv_batch = 1.0f / (float)batch;
    for (int s = 0; train && s < n_steps; ++s) {
        // ---- the minibatch: rows >= batch are zero rows with a zero loss gradient ----
        if (tid < kLearnRows) {
            int slot = 0;
            if (tid < batch) {
                if (A.slots) slot = A.slots[((size_t)brain * n_steps + s) * batch + tid];
                else slot = (int)(((uint64_t)rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)calls, (uint32_t)kLearnSite, (uint32_t)(s * batch + tid)).x * (uint64_t)size) >> 32);
            }
            row_slot[tid] = tid < batch ? slot : -1;
            row_a[tid] = tid < batch ? (int)B.r_action[slot] & 7 : 0;
            row_r[tid] = tid < batch ? B.r_reward[slot] : 0.0f;
            row_mask[tid] = tid < batch ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
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
        learn_forward<153, 128, kXS, kH1S, true>(B.target + oW1, B.target + oB1, xp, h1, tid);
        __syncthreads();
        learn_forward<128, 64, kH1S, kH2S, true>(B.target + oW2, B.target + oB2, h1, h2, tid);
        __syncthreads();
        learn_forward<64, 8, kH2S, 8, false>(B.target + oW3, B.target + oB3, h2, q, tid);
        __syncthreads();
        if (tid < kLearnRows) {
            float mx = q[tid * 8];
            for (int a = 1; a < 8; ++a) mx = fmaxf(mx, q[tid * 8 + a]);
            row_loss[tid] = mx;
        }
        __syncthreads();
        // ---- Q_eval(s) ----
        learn_forward<153, 128, kXS, kH1S, true>(B.params + oW1, B.params + oB1, xs, h1, tid);
        __syncthreads();
        learn_forward<128, 64, kH1S, kH2S, true>(B.params + oW2, B.params + oB2, h1, h2, tid);
        __syncthreads();
        learn_forward<64, 8, kH2S, 8, false>(B.params + oW3, B.params + oB3, h2, q, tid);
        __syncthreads();
        // ---- smooth-L1 (beta = 1) of q[a] against r + gamma max q' done_mask, and its gradient ----
        if (tid < kLearnRows) {
            const float target = row_r[tid] + (B.gamma * row_loss[tid]) * row_mask[tid];
            const float td = q[tid * 8 + row_a[tid]] - target, ad = fabsf(td);
            const bool in = tid < batch;
            row_loss[tid] = in ? (ad < 1.0f ? (0.5f * td) * td : ad - 0.5f) : 0.0f;
            row_g[tid] = in ? fminf(fmaxf(td, -1.0f), 1.0f) * inv_batch : 0.0f;
        }
        __syncthreads();
        if (tid == 0 && B.loss) {
            float sum = 0.0f;
            for (int j = 0; j < kLearnRows; ++j) sum += row_loss[j];
            B.loss[s] = sum * inv_batch;
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
        // ---- gradients and Adam, parameter by parameter (nothing below reads a parameter of this network) ----
        const double t = (double)(steps_taken + 1);
        AdamStep ad;
        ad.p = B.params; ad.m = B.adam_m; ad.v = B.adam_v;
        ad.grad = B.grad ? B.grad + (size_t)s * kNParams : nullptr;
        ad.w1 = 1.0 - B.beta1; ad.w2 = 1.0 - B.beta2; ad.beta2 = B.beta2; ad.eps = B.eps_d;
        ad.bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
        ad.neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
        learn_wgrad<153, 128, kH1S, kXS>(ad, oW1, d1, xs, tid);
        learn_bgrad<128, kH1S>(ad, oB1, d1, tid);
        learn_wgrad<128, 64, kH2S, kH1S>(ad, oW2, d2, h1, tid);
        learn_bgrad<64, kH2S>(ad, oB2, d2, tid);
        for (int item = tid; item < 8 * 64; item += kLearnBlock) {   // fc3: only the taken action's row of a minibatch row is non-zero
            const int a = item >> 6, k = item & 63;
            float g = 0.0f;
#pragma unroll 4
            for (int row = 0; row < kLearnRows; ++row) g = fmaf(row_a[row] == a ? row_g[row] : 0.0f, h2[row * kH2S + k], g);
            adam_update(ad, oW3 + item, g);
        }
        if (tid < 8) {
            float g = 0.0f;
            for (int row = 0; row < kLearnRows; ++row) g += row_a[row] == tid ? row_g[row] : 0.0f;
            adam_update(ad, oB3 + tid, g);
        }
        ++steps_taken;
        __syncthreads();   // the next step (and the packer) read the new parameters
    }
    if (B.sync_target)     // DQN.py:83: after every train(), also below the size gate
        for (int i = tid; i < kNParams; i += kLearnBlock) B.target[i] = B.params[i];
    if (tid == 0) { B.state[0] = steps_taken; B.state[1] = calls + 1; }
    learn_pack_dqn(B.params, B.packed, sc, un, tid);
}


// ---- minibatch draws that do not depend on the ORDER of a ring (rl_learn_draw) ----
// The multi-tick launch appends every world's transitions with an atomic add on the ring's counter: the SET of transitions a ring holds
// repeats from run to run, their slots do not.  So a draw must not name a slot.  Every row gets a 64-bit key of its CONTENT (a sum of
// mixed (position, bits) terms: any summation order gives the same key), and draw d takes the row whose key, mixed with the draw's own
// 64 Philox bits, is smallest (ties: equal keys are equal rows up to a 2^-64 collision; the lower slot).  For a fixed set of distinct
// keys the minimum of a well-mixed key is uniform over the rows and independent between draws -- as far as mix64 behaves like a random
// function: an empirical property (tests/test_hip_learn.py counts 6,400 draws over 48 rows), not a proven one.  Sampling with replacement,
// the same rows whatever slots they sit in.
struct DrawBrain {
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const int32_t* r_age;
    const unsigned long long* r_count;
    long long r_capacity;
    unsigned long long* keys;    // [capacity]
    const long long* state;      // rl_learner.state ([1] = calls made)
    int batch;
};
struct DrawArgs {
    DrawBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* slots;              // [n_learners][n_steps][batch]
    uint64_t seed;
    int n_steps;
};
// one wave per ring row: keys[row] = sum of the terms of state (positions 0..152), state_prime (153..305), action, reward, done, age
__global__ __launch_bounds__(256) void k_learn_keys(const DrawArgs A)
{
    const DrawBrain& B = A.b[blockIdx.y];
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= size) return;
    const uint64_t k = learn_row_key(B.r_state, B.r_state_prime, B.r_action, B.r_reward, B.r_done, B.r_age, row, lane);
    if (lane == 0) B.keys[row] = k;
}

// one workgroup per draw: slots[brain][d] = argmin over rows of mix(key ^ salt_d)
__global__ __launch_bounds__(256) void k_learn_pick(const DrawArgs A)
{
    __shared__ uint64_t best_v[256];
    __shared__ int best_i[256];
    const int brain = blockIdx.y, d = blockIdx.x, tid = threadIdx.x;
    const DrawBrain& B = A.b[brain];
    if (d >= A.n_steps * B.batch) return;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const rl_u4 r = rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)B.state[1], (uint32_t)kLearnSite, (uint32_t)d);
    const uint64_t salt = ((uint64_t)r.y << 32) | r.x;
    uint64_t bv = ~0ull;
    int bi = 0x7fffffff;
    for (long long i = tid; i < size; i += 256) {   // (ascending i per thread: the first of equal values stays)
        const uint64_t v = learn_mix64(B.keys[i] ^ salt);
        if (v < bv) { bv = v; bi = (int)i; }
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
    if (tid == 0) {
        int batch0 = 0;   // (the learners' rows of `slots` are [n_steps][batch] each, laid end to end)
        for (int b = 0; b < brain; ++b) batch0 += A.n_steps * A.b[b].batch;
        A.slots[batch0 + d] = size > 0 ? best_i[0] : 0;
    }
}

}  // namespace

int rl_learn_supported_impl(int kind) { return kind == RL_DQN ? 1 : 0; }

int rl_learn_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
                    hipStream_t stream)
{
    LearnArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        LearnBrain& b = a.b[i];
        b.params = l.params; b.target = l.target; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.packed = l.packed; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2);
        b.gamma = l.gamma; b.eps_d = learn_decimal(l.eps);
        b.batch = l.batch; b.min_size = l.min_size; b.sync_target = l.sync_target;
    }
    a.slots = slots; a.err = h->err_flag; a.seed = h->cfg.seed; a.n_steps = n_steps;
    {   // the large dynamic-LDS window (93 KB): asked for at every call -- idempotent, host-only, and right on whatever device is current
        const hipError_t e = hipFuncSetAttribute((const void*)k_learn_dqn, hipFuncAttributeMaxDynamicSharedMemorySize, kLearnLdsBytes);
        if (e != hipSuccess) { rl_set_error("rl_learn: hipFuncSetAttribute(%d bytes of LDS) failed: %s", kLearnLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    hipLaunchKernelGGL(k_learn_dqn, dim3(n_learners), dim3(kLearnBlock), kLearnLdsBytes, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

int rl_learn_draw_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps,
                         unsigned long long* const* keys, int32_t* slots, hipStream_t stream)
{
    DrawArgs a{};
    long long max_cap = 1;
    int max_batch = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        DrawBrain& b = a.b[i];
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done; b.r_age = r.age;
        b.r_count = r.count; b.r_capacity = r.capacity; b.keys = keys[i]; b.state = (const long long*)learners[i].state; b.batch = learners[i].batch;
        max_cap = r.capacity > max_cap ? r.capacity : max_cap;
        max_batch = b.batch > max_batch ? b.batch : max_batch;
    }
    a.slots = slots; a.seed = h->cfg.seed; a.n_steps = n_steps;
    hipLaunchKernelGGL(k_learn_keys, dim3((unsigned)((max_cap + 3) / 4), n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_learn_pick, dim3(n_steps * max_batch, n_learners), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_draw: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}
