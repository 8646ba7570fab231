// rl_learn_ppo.hip -- k_learn_ppo: the PPO brain's rollouts on the device (rl_learn_ppo), and the on-policy draw that names their rows
// (rl_learn_rollout: k_rollout_prepare, k_rollout_pick), from the replay rings rl_run_ex / rl_capture_transitions fill to the packed
// weights the acting kernels read, with no host round trip.
//
// Reference (ReinLife/Models/PPO.py):
//   PPOAgent.learn     :71-77     appends (s, a, reward / 100.0, s', prob[a], done); trains on the whole list and empties it
//   PPO.learn          :136-162   k_epoch full-batch Adam steps, each from the current parameters:
//                                   td = r + gamma v(s') (1 - done); delta = td - v(s), detached
//                                   adv_t = gamma lmbda adv_{t+1} + delta_t, backwards over the list, NO reset at done (float32 under
//                                   numpy 2: the double gamma * lmbda rounded to float, one multiply, one add, no fma)
//                                   ratio = exp(log pi(s)[a] - log prob_a); surr1 = ratio adv; surr2 = clamp(ratio, 1 - eps, 1 + eps) adv
//                                   loss = mean_i(-min(surr1, surr2)_i) + smooth_l1(v(s), td)   (the second term is a mean already)
//   PPO.pi / PPO.v     :101-112   fc1 153 -> 256, fc2 256 -> 256, fc_pi 256 -> 8 (softmax), fc_v 256 -> 1, ReLU after fc1 and fc2:
//                                 107,529 parameters in state-dict order
//   torch.optim.Adam   betas (0.9, 0.999), eps 1e-8 (:99)
// Gradients, as torch makes them: nothing flows through v(s') or the advantage; dL/dv_i = clamp(v_i - td_i, -1, 1) / T;
// min(a, b) gives the smaller side the whole gradient and each side half at a == b; clamp passes gradient on [1 - eps, 1 + eps], bounds
// included: dL/dratio_i = -(adv_i / T) ([s1 < s2] + 1/2 [s1 == s2] + in_i ([s2 < s1] + 1/2 [s1 == s2])); dratio/dlogit_j = ratio ([j == a] - pi_j).
//
// Shape.  One 512-thread workgroup per learning brain makes the call's n_steps rollouts one after the other, k_epoch Adam steps each;
// workgroups never meet.  Plain f32 FMA, every sum by ONE thread in a fixed order (k or row ascending), no float atomics: the same
// buffers give the same bits whatever else is in the launch.  The per-row scalars (softmax, ratio, losses: 32 rows, one thread each) are
// formed in double from the f32 logits and rounded once; the GAE recursion is one thread's, in float32 as the reference's.
//
// Weights come through coalesced LDS tiles as in k_learn_d3qn (rl_learn_dueling.hip), the next tile's loads in flight: y = W x tiles of 256
// outputs x 32 k (rows padded to 36 floats), W^T d tiles of 32 outputs x 256 k.  A thread owns 4 rows x 4 outputs.
//
// LDS (about 125 KB dynamic), 32 rollout rows:
//   S   [32][160]  s' for the value pass, then s (kept until fc1's weight gradient)
//   H1  [32][256]  relu(fc1)
//   H2  [32][256]  relu(fc2), overwritten IN PLACE by its back-propagated rows d2 once the heads' gradients are summed (registers)
//   WT  36,864 B   the weight tile; after the backward pass through fc2 it holds d1 [32][256]; the packer's feature scales at the end
//   logits [32][8] (then dL/dlogit), per-row scalars
// All back-propagated rows are complete before the first parameter changes; each parameter gets its Adam update (rl_learn_dev.h: the
// double update of k_learn_d3qn) from the thread that summed its gradient.
//
// Packing.  After the last rollout the workgroup rewrites `packed` from the final parameters: rl_policy.hip's pack_in_layer 153 -> 256,
// pack_hidden_layer 256 -> 256 and pack_head 256 -> 8 at Layout.l1 / l2a / ha, bit for bit (fc_v is not packed: acting never reads it).
#include "rl_learn_dev.h"

#include <math.h>

namespace {

constexpr int kPBlock = 512;
constexpr int kPRows = RL_PPO_ROLLOUT_MAX;     // rows of a rollout at most (rl_learner.batch)
constexpr int kPS = 160, kPH = 256;            // LDS row strides in floats (153 / 256 used; columns 153..159 of S are zero)
constexpr int kPWTS = 36;                      // row stride of a forward weight tile [256][32]
constexpr int kPWTFloats = 256 * kPWTS;        // (>= the backward tile's 32 * 256 and d1's 32 * 256)
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
constexpr int kRolloutSite = RL_SITE_LEARN_ROLLOUT;
// state-dict-flat offsets (fc1, fc2, fc_pi, fc_v: weight then bias each)
constexpr int oW1 = 0, oB1 = 153 * 256, oW2 = oB1 + 256, oB2 = oW2 + 256 * 256, oWp = oB2 + 256, oBp = oWp + 8 * 256, oWv = oBp + 8,
              oBv = oWv + 256, kNParams = oBv + 1;
static_assert(kNParams == 107529, "the PPO network has 107,529 parameters");
constexpr int kNHead = kNParams - oWp;         // fc_pi.weight, fc_pi.bias, fc_v.weight, fc_v.bias: contiguous, 2,313
constexpr int kHeadRegs = (kNHead + kPBlock - 1) / kPBlock;
constexpr int kNFeat = 256 + 256 + 8;          // output features of the three packed layers (the packer's scales)
static_assert(kPRows == 32, "k_learn_ppo's tiles are written for 32 rows");
static_assert(2 * kNFeat <= kPWTFloats && kPRows * kPH <= kPWTFloats, "the packer's scales and d1 live in the weight tile");

struct PpoBrain {
    float *params, *adam_m, *adam_v;
    long long* state;
    float* packed;
    float* loss;
    float* grad;
    const float *r_state, *r_state_prime, *r_reward, *r_prob;
    const int8_t* r_action;
    const uint8_t* r_done;
    const unsigned long long* r_count;
    const unsigned long long* fresh;   // rl_ppo.fresh or null
    long long r_capacity;
    double lr, beta1, beta2, eps_d;    // the decimal values the caller's floats stand for (learn_decimal)
    float gamma, gl, clip_lo, clip_hi; // gl = (float)(gamma * lmbda), the bounds (float)(1 -+ eps_clip): from the decimals, as Python makes them
    int batch, k_epoch;
};
struct PpoArgs {
    PpoBrain b[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;              // [n_learners][n_steps][batch]
    int32_t* err;
    int n_steps;
};

constexpr int kPLdsFloats = kPRows * kPS + 2 * kPRows * kPH + kPWTFloats + kPRows * 8 * 2 + 12 * kPRows;
constexpr int kPLdsBytes = kPLdsFloats * 4;
static_assert(kPLdsBytes + 1024 <= 160 * 1024, "k_learn_ppo's LDS map must fit a workgroup's 160 KiB");

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

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending) and Adam at once, for a layer of 256 outputs.  A work item is 4 outputs x 4
// consecutive k; consecutive threads take consecutive k groups.
template <int NIN, int INS>
__device__ __forceinline__ void ppo_wgrad(const AdamStep& a, int off, const float* D, const float* IN, int tid)
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
                if (4 * kg + j < NIN) adam_update(a, off + (4 * og + i) * NIN + 4 * kg + j, acc[i][j]);
    }
}
__device__ __forceinline__ void ppo_bgrad(const AdamStep& a, int off, const float* D, int tid)
{
    if (tid < 256) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kPRows; ++row) g += D[row * kPH + tid];
        adam_update(a, off + tid, g);
    }
}

// the rollout's rows of `src` (state or state_prime of the ring) -> X [32][160]; rows without a slot and columns >= 153 are zero
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

// ---- rl_policy_pack_weights(RL_PPO, P) -> packed, by the whole workgroup.  sc / un: LDS [kNFeat] each, features of fc1 | fc2 | fc_pi ----
__device__ __forceinline__ void ppo_pack_consts(const float* bias, const float* un, float* consts, int tid)   // write_epilogue_consts, 8 output tiles
{
    for (int ii = tid; ii < 512; ii += kPBlock) {
        const int r = ii & 15, th = ii >> 5;
        const int o = 32 * (th >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (th & 1);
        consts[ii] = (ii & 16) ? bias[o] : un[o];
    }
}
__device__ __forceinline__ void ppo_pack(const float* P, float* packed, float* sc, float* un, int tid)
{
    const Layout L = layout_of(RL_PPO);
    for (int f = tid; f < kNFeat; f += kPBlock) {   // feature_scales: 2^(kScaleExp - exponent(max |W[o][:]|))
        const int n_in = f < 256 ? 153 : 256;
        const float* w = f < 256 ? P + oW1 + f * 153 : f < 512 ? P + oW2 + (f - 256) * 256 : P + oWp + (f - 512) * 256;
        float mx = 0.0f;
#pragma unroll 4
        for (int k = 0; k < n_in; ++k) mx = fmaxf(mx, fabsf(w[k]));
        row_scale(mx, sc[f], un[f]);
    }
    __syncthreads();
    uint4* d1 = (uint4*)(packed + L.l1);
    for (int u = tid; u < kInChunks * 8 * 64; u += kPBlock) {        // pack_in_layer 153 -> 256: [c][t][plane][lane]
        const int lane = u & 63, t = (u >> 6) & 7, c = u >> 9;
        const int o = 32 * t + (lane & 31), k0 = 16 * c + 8 * (lane >> 5);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = k0 + e < 153 ? P[oW1 + o * 153 + k0 + e] * sc[o] : 0.0f;
        uint4* dst = d1 + ((c * 8 + t) * kPlanes) * 64 + lane;
        learn_store_fragment(x, dst, dst + 64);
    }
    ppo_pack_consts(P + oB1, un, packed + L.l1 + frag_floats(kInChunks, 8), tid);
    uint4* d2 = (uint4*)(packed + L.l2a);
    for (int u = tid; u < 16 * 8 * 64; u += kPBlock) {               // pack_hidden_layer 256 -> 256: [s = 2t + c][t2][plane][lane]
        const int lane = u & 63, t2 = (u >> 6) & 7, s = u >> 9;
        const int o = 32 * t2 + (lane & 31);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = P[oW2 + o * 256 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[256 + o];
        uint4* q = d2 + ((s * 8 + t2) * kPlanes) * 64 + lane;
        learn_store_fragment(x, q, q + 64);
    }
    ppo_pack_consts(P + oB2, un + 256, packed + L.l2a + frag_floats(16, 8), tid);
    uint4* dh = (uint4*)(packed + L.ha);
    for (int u = tid; u < 16 * 64; u += kPBlock) {                   // pack_head 256 -> 8: [2t + c][plane][lane], rows >= 8 zero
        const int lane = u & 63, s = u >> 6;
        const int o = lane & 31;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = o < 8 ? P[oWp + o * 256 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[512 + o] : 0.0f;
        uint4* q = dh + (s * kPlanes) * 64 + lane;
        learn_store_fragment(x, q, q + 64);
    }
    if (tid < 16) packed[L.ha + head_consts_off(8) + tid] = tid < 8 ? un[512 + tid] : P[oBp + tid - 8];
}

__global__ __launch_bounds__(kPBlock) void k_learn_ppo(const PpoArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float ppo_lds[];
    float* xs = ppo_lds;                            // S  [32][160]
    float* h1 = xs + kPRows * kPS;                  // H1 [32][256]
    float* h2 = h1 + kPRows * kPH;                  // H2 [32][256]  (d2)
    float* wt = h2 + kPRows * kPH;                  // weight tile (d1 [32][256]; the packer's sc / un)
    float* lg = wt + kPWTFloats;                    // [32][8] logits, then dL/dlogit
    float* pi = lg + kPRows * 8;                    // [32][8] softmax
    float* row_v = pi + kPRows * 8;                 // [32] v(s)
    float* row_vp = row_v + kPRows;                 // [32] v(s')
    float* row_r = row_vp + kPRows;                 // [32] reward / 100
    float* row_mask = row_r + kPRows;               // [32] 1 - done
    float* row_pb = row_mask + kPRows;              // [32] prob_a
    float* row_ratio = row_pb + kPRows;             // [32]
    float* row_td = row_ratio + kPRows;             // [32]
    float* row_delta = row_td + kPRows;             // [32]
    float* row_adv = row_delta + kPRows;            // [32]
    float* row_gv = row_adv + kPRows;               // [32] dL/dv
    float* row_l = row_gv + kPRows;                 // [32] the row's two loss terms added (as float pairs: row_l, row_l2)
    float* row_l2 = row_l + kPRows;                 // [32]
    __shared__ int first_bad;
    __shared__ int row_slot[kPRows];
    __shared__ int row_a[kPRows];

    const int tid = threadIdx.x, brain = blockIdx.x;
    const PpoBrain& B = A.b[brain];
    const int batch = B.batch, n_steps = A.n_steps, k_epoch = B.k_epoch;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const long long calls = B.state[1];
    long long steps_taken = B.state[0];
    const bool train = !(B.fresh && *B.fresh == 0ull);   // `if self.data()` (PPO.py:76): an empty window makes no update

    if (train) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        const int32_t* sl = A.slots + (size_t)brain * n_steps * batch;
        for (int i = tid; i < n_steps * batch; i += kPBlock)
            if (sl[i] < 0 || sl[i] >= size) atomicMin(&first_bad, i);
        __syncthreads();
        const int bad = first_bad;
        if (bad != 0x7fffffff) {
            if (tid == 0 && A.err && atomicCAS(A.err, 0, kErrLearnSlot) == 0) { A.err[1] = brain; A.err[2] = bad / batch; A.err[3] = sl[bad]; }
            return;   // (uniform) this brain's buffers stay exactly as they were
        }
    }
    for (int s = 0; train && s < n_steps; ++s) {
        // ---- the rollout: rows >= batch are zero rows with zero loss gradients, and stay out of every mean and of the GAE ----
        __syncthreads();
        if (tid < kPRows) {
            const bool in = tid < batch;
            const int slot = in ? A.slots[((size_t)brain * n_steps + s) * batch + tid] : 0;
            row_slot[tid] = in ? slot : -1;
            row_a[tid] = in ? (int)B.r_action[slot] & 7 : 0;
            row_r[tid] = in ? (float)((double)B.r_reward[slot] / 100.0) : 0.0f;   // PPO.py:73
            row_mask[tid] = in ? (B.r_done[slot] ? 0.0f : 1.0f) : 0.0f;
            row_pb[tid] = in ? B.r_prob[slot] : 1.0f;
        }
        __syncthreads();
        for (int ep = 0; ep < k_epoch; ++ep) {
            // The buffers' addresses are re-read as opaque values in every epoch: otherwise the compiler hoists the per-lane addresses of every
            // parameter access of the epoch (hundreds of 64-bit values) in front of the loops and spills them.
            typedef float __attribute__((address_space(1))) gf;   // (global pointers stay global pointers through the asm)
            gf *gP = (gf*)B.params, *gAM = (gf*)B.adam_m, *gAV = (gf*)B.adam_v, *gGR = (gf*)B.grad;
            const gf *gRS = (const gf*)B.r_state, *gRSP = (const gf*)B.r_state_prime;
            asm volatile("" : "+s"(gP), "+s"(gAM), "+s"(gAV), "+s"(gGR), "+s"(gRS), "+s"(gRSP));
            float *P = (float*)gP, *AM = (float*)gAM, *AV = (float*)gAV, *GR = (float*)gGR;
            const float *RS = (const float*)gRS, *RSP = (const float*)gRSP;
            // ---- v(s'): the trunk and fc_v on the s' rows ----
            ppo_stage_rows(RSP, row_slot, xs, tid);
            ppo_forward<153, kPS>(P + oW1, P + oB1, xs, h1, wt, tid);
            ppo_forward<256, kPH>(P + oW2, P + oB2, h1, h2, wt, tid);
            if (tid < kPRows) row_vp[tid] = ppo_dot256(P + oWv, P[oBv], h2 + tid * kPH);
            __syncthreads();
            // ---- the trunk and both heads on the s rows ----
            ppo_stage_rows(RS, row_slot, xs, tid);
            ppo_forward<153, kPS>(P + oW1, P + oB1, xs, h1, wt, tid);
            ppo_forward<256, kPH>(P + oW2, P + oB2, h1, h2, wt, tid);
            if (tid < kPRows * 8) lg[tid] = ppo_dot256(P + oWp + (tid & 7) * 256, P[oBp + (tid & 7)], h2 + (tid >> 3) * kPH);
            else if (tid < kPRows * 9) row_v[tid - kPRows * 8] = ppo_dot256(P + oWv, P[oBv], h2 + (tid - kPRows * 8) * kPH);
            __syncthreads();
            // ---- softmax, ratio, td, delta (one thread per row) ----
            if (tid < kPRows) {
                const float* l = lg + tid * 8;
                float mx = l[0];
                for (int a = 1; a < 8; ++a) mx = fmaxf(mx, l[a]);
                double e[8], sum = 0.0;
                for (int a = 0; a < 8; ++a) { e[a] = exp((double)l[a] - (double)mx); sum += e[a]; }
                for (int a = 0; a < 8; ++a) pi[tid * 8 + a] = (float)(e[a] / sum);
                const int a = row_a[tid];
                row_ratio[tid] = (float)exp(((double)l[a] - (double)mx - log(sum)) - log((double)row_pb[tid]));
                const float td = row_r[tid] + (B.gamma * row_vp[tid]) * row_mask[tid];
                row_td[tid] = td;
                row_delta[tid] = td - row_v[tid];
            }
            __syncthreads();
            // ---- GAE, backwards over the rollout's rows, no reset at done: float32, one multiply, one add, no fma (PPO.py:144-150) ----
            if (tid == 0) {
                float adv = 0.0f;
                for (int t = batch - 1; t >= 0; --t) {
                    adv = __fadd_rn(__fmul_rn(B.gl, adv), row_delta[t]);
                    row_adv[t] = adv;
                }
            }
            __syncthreads();
            // ---- the losses and dL/dratio, dL/dv per row ----
            if (tid < kPRows) {
                const bool in = tid < batch;
                const float ratio = row_ratio[tid], adv = row_adv[tid];
                const float s1 = ratio * adv;
                const float s2 = fminf(fmaxf(ratio, B.clip_lo), B.clip_hi) * adv;
                const float inside = (ratio >= B.clip_lo && ratio <= B.clip_hi) ? 1.0f : 0.0f;
                const float coef = s1 < s2 ? 1.0f : s2 < s1 ? inside : 0.5f + 0.5f * inside;
                const float gr = in ? -(adv / (float)batch) * coef : 0.0f;
                const float d = row_v[tid] - row_td[tid];
                const float ad = fabsf(d);
                row_l[tid] = in ? -fminf(s1, s2) : 0.0f;
                row_l2[tid] = in ? (ad < 1.0f ? 0.5f * d * d : ad - 0.5f) : 0.0f;
                row_gv[tid] = in ? fminf(fmaxf(d, -1.0f), 1.0f) / (float)batch : 0.0f;
                const float g = gr * ratio;
                const int a = row_a[tid];
                for (int j = 0; j < 8; ++j) lg[tid * 8 + j] = in ? g * ((j == a ? 1.0f : 0.0f) - pi[tid * 8 + j]) : 0.0f;
            }
            __syncthreads();
            if (tid == 0 && B.loss) {
                double sum = 0.0, sum2 = 0.0;
                for (int j = 0; j < batch; ++j) { sum += (double)row_l[j]; sum2 += (double)row_l2[j]; }
                B.loss[s * k_epoch + ep] = (float)(sum / (double)batch + sum2 / (double)batch);
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
            // ---- gradients and Adam, parameter by parameter (nothing below reads a parameter) ----
            const double t = (double)(steps_taken + 1);
            AdamStep ad;
            ad.p = P; ad.m = AM; ad.v = AV;
            ad.grad = GR ? GR + (size_t)(s * k_epoch + ep) * kNParams : nullptr;
            ad.w1 = 1.0 - B.beta1; ad.w2 = 1.0 - B.beta2; ad.beta2 = B.beta2; ad.eps = B.eps_d;
            ad.bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
            ad.neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
#pragma unroll
            for (int p = 0; p < kHeadRegs; ++p) {
                const int idx = tid + kPBlock * p;
                if (idx < kNHead) adam_update(ad, oWp + idx, head_g[p]);
            }
            ppo_wgrad<256, kPH>(ad, oW2, h2, h1, tid);
            ppo_bgrad(ad, oB2, h2, tid);
            ppo_wgrad<153, kPS>(ad, oW1, wt, xs, tid);
            ppo_bgrad(ad, oB1, wt, tid);
            ++steps_taken;
            __syncthreads();   // the next epoch (and the packer) read the new parameters
        }
    }
    if (tid == 0) { B.state[0] = steps_taken; B.state[1] = calls + 1; }
    ppo_pack(B.params, B.packed, wt, wt + kNFeat, tid);
}

// ---- rl_learn_rollout: the on-policy draw.  The window is the rows appended since the last call, slots [seen, count) mod capacity (the
// whole ring once count - seen >= capacity); draw d takes the window row whose content key (learn_row_key, unchanged), mixed with the
// draw's own 64 Philox bits, is smallest: uniform over the fresh rows, with replacement, the same rows whatever slots they sit in.
// k_rollout_prepare reads `seen`, writes the window's keys and *fresh; k_rollout_pick, a later launch, finds the window from *fresh and
// the ring's count alone, and advances *seen to the count. ----
struct RollBrain {
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const int32_t* r_age;
    const unsigned long long* r_count;
    long long r_capacity;
    unsigned long long *keys, *seen, *fresh;
    const long long* state;      // rl_learner.state ([1] = calls made)
    int batch;
};
struct RollArgs {
    RollBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* slots;              // the learners' [n_steps][batch] tables, end to end
    uint64_t seed;
    int n_steps;
};

__device__ inline unsigned long long rollout_fresh(unsigned long long count, unsigned long long seen, unsigned long long cap)
{
    const unsigned long long f = count > seen ? count - seen : 0ull;
    return f < cap ? f : cap;
}

// one wave per ring row: keys[row] for the rows of the window
__global__ __launch_bounds__(256) void k_rollout_prepare(const RollArgs A)
{
    const RollBrain& B = A.b[blockIdx.y];
    const unsigned long long count = *B.r_count, seen = *B.seen, cap = (unsigned long long)B.r_capacity;
    const unsigned long long fresh = rollout_fresh(count, seen, cap);
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
__global__ __launch_bounds__(256) void k_rollout_pick(const RollArgs A)
{
    __shared__ uint64_t best_v[256];
    __shared__ int best_i[256];
    const int brain = blockIdx.y, d = blockIdx.x, tid = threadIdx.x;
    const RollBrain& B = A.b[brain];
    if (d >= A.n_steps * B.batch) return;
    const unsigned long long count = *B.r_count, cap = (unsigned long long)B.r_capacity;
    unsigned long long fresh = *B.fresh;   // (k_rollout_prepare wrote it in the launch in front of this one)
    if (fresh > cap) fresh = cap;
    if (fresh > count) fresh = count;
    const unsigned long long first = (count - fresh) % cap;
    if (d == 0 && tid == 0) *B.seen = count;   // (k_rollout_prepare is its only reader)
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
    if (tid == 0) {
        int batch0 = 0;   // (the learners' rows of `slots` are [n_steps][batch] each, laid end to end)
        for (int b = 0; b < brain; ++b) batch0 += A.n_steps * A.b[b].batch;
        A.slots[batch0 + d] = (fresh > 0 && best_i[0] != 0x7fffffff) ? best_i[0] : 0;
    }
}

}  // namespace

int rl_learn_ppo_supported_impl(int kind) { return kind == RL_PPO ? 1 : 0; }

int rl_learn_ppo_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                        const int32_t* slots, hipStream_t stream)
{
    PpoArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        PpoBrain& b = a.b[i];
        b.params = l.params; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.packed = l.packed; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_prob = r.prob; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity; b.fresh = ppos[i].fresh;
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2); b.eps_d = learn_decimal(l.eps);
        const double gamma = learn_decimal(l.gamma), lmbda = learn_decimal(ppos[i].lmbda), clip = learn_decimal(ppos[i].eps_clip);
        b.gamma = (float)gamma; b.gl = (float)(gamma * lmbda); b.clip_lo = (float)(1.0 - clip); b.clip_hi = (float)(1.0 + clip);
        b.batch = l.batch; b.k_epoch = ppos[i].k_epoch;
    }
    a.slots = slots; a.err = h->err_flag; a.n_steps = n_steps;
    {   // the large dynamic-LDS window (125 KB): asked for at every call -- idempotent, host-only, and right on whatever device is current
        const hipError_t e = hipFuncSetAttribute((const void*)k_learn_ppo, hipFuncAttributeMaxDynamicSharedMemorySize, kPLdsBytes);
        if (e != hipSuccess) { rl_set_error("rl_learn_ppo: hipFuncSetAttribute(%d bytes of LDS) failed: %s", kPLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    hipLaunchKernelGGL(k_learn_ppo, dim3(n_learners), dim3(kPBlock), kPLdsBytes, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_ppo: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

int rl_learn_rollout_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                            int32_t* slots, hipStream_t stream)
{
    RollArgs a{};
    long long max_cap = 1;
    int max_batch = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        RollBrain& b = a.b[i];
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done; b.r_age = r.age;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.keys = ppos[i].keys; b.seen = ppos[i].seen; b.fresh = ppos[i].fresh;
        b.state = (const long long*)learners[i].state; b.batch = learners[i].batch;
        max_cap = r.capacity > max_cap ? r.capacity : max_cap;
        max_batch = b.batch > max_batch ? b.batch : max_batch;
    }
    a.slots = slots; a.seed = h->cfg.seed; a.n_steps = n_steps;
    hipLaunchKernelGGL(k_rollout_prepare, dim3((unsigned)((max_cap + 3) / 4), n_learners), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_rollout: launch of the prepare kernel failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    hipLaunchKernelGGL(k_rollout_pick, dim3(n_steps * max_batch, n_learners), dim3(256), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_rollout: launch of the pick kernel failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}
