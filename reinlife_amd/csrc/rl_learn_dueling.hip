// rl_learn_dueling.hip -- k_learn_d3qn: the D3QN brain's minibatch updates on the device, from the replay rings rl_run_ex /
// rl_capture_transitions fill to the packed weights the acting kernels read, with no host round trip.
//
// Reference (paths under ReinLife/Models):
//   D3QNAgent.train             D3QN.py:97-116   sample 64, MSE of q[a] against r + gamma (1 - done) max q'_target(s'), ONE Adam step
//   D3QNAgent.learn             D3QN.py:118-126  the caller's schedule: train only once n_epi > exploration, target <- eval every
//                                                soft_update_freq episodes (rl_learner.sync_target)
//   dueling_ddqn.forward        D3QN.py:161-165  fc 153 -> 128, two branches 128 -> 128 -> 8 / 1, ReLU between,
//                                                q = advantage + value - advantage.mean(): the mean of the WHOLE minibatch's advantages,
//                                                not of a row's (the acting path's per-row mean is the same expression at batch 1)
//   torch.optim.Adam            betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad (D3QN.py:61)
//
// Shape.  One 512-thread workgroup (two waves per SIMD) per learning brain makes the call's n_steps updates one after the other;
// workgroups never meet.  Arithmetic is plain f32 FMA, every sum in a fixed order: a dot product by ONE thread, k (or row) ascending;
// the batch-wide mean as 64 row sums (one thread each, action ascending) added by one thread, row ascending.  No float atomics.  Same
// buffers, same bits, whatever else is in the launch.  (FMA rather than the matrix pipe or the 2 x f16 split: DESIGN.md 5.17.)
//
// Weights.  Every weight matrix is read from global memory with consecutive lanes on consecutive addresses, into an LDS tile that the
// whole workgroup then reads: for y = W x tiles of 128 outputs x 32 k (rows padded to 36 floats: a lane's four outputs are 32 apart, so
// the sixteen lanes of a 16-byte LDS read sit on distinct banks), for the backward W^T d tiles of 32 outputs x 128 k.  The next tile's
// loads are in flight while the current one is used.  The weight gradients read both operands from LDS and update each parameter by
// the thread that summed it: consecutive lanes own consecutive k, so the parameters' and moments' traffic is contiguous too.
//
// LDS (161,280 bytes dynamic and 528 static of the workgroup's 163,840), 64 minibatch rows:
//   A   [64][160]  s' for the target forward (which keeps only max q'), then s for the eval forward; dead after fc's forward, so the
//                  back-propagated rows of fc, d_f [64][128], are written here
//   F   [64][128]  relu(fc) of the network being evaluated
//   HA  [64][128]  relu(adv_fc1), overwritten IN PLACE by its back-propagated rows da once the head gradients are taken
//   HV  [64][128]  relu(value_fc1), likewise dv
//                  HA and HV together take the minibatch's s rows again (from the ring: 39 KB, L2-resident) for fc's weight gradient,
//                  after the two branches' weight gradients are done with them
//   WT  18,432 B   the weight tile; the packer's feature scales at the end of the call
//   adv [64][8] (then dL/dadv), val [64], per-row scalars
// The gradients of the two heads (1,161 parameters) are summed before da / dv overwrite HA / HV and held in registers (at most three
// per thread) until their Adam update.  All back-propagated rows are complete before the first parameter changes.
//
// Prioritised memory (k_learn_d3qn<true>, rl_learn_prioritized).  PERD3QNAgent.train() (PERD3QN.py:94-115) is this update with one
// addition: the loss is the same plain nn.MSELoss (PERD3QN.py:56, 109 -- sample()'s importance weights are computed and never used), and
// after the forward passes every batch row's priority becomes |max_a q'_target(s') - q_eval(s)[a]| (PERD3QN.py:110-111: the reference's
// expression, not the TD error).  The thread that forms a row's td writes priority[slot] from the same two numbers; duplicated slots write
// equal bits.  After the last step of a call that trained the workgroup leaves max(priority[0 .. size)) in *prio_max: what store() gives
// the next new rows (PERD3QN.py:147).  The maximum is over the rows as they stand: the caller has drawn (and so stamped the new rows)
// since the last append -- the order rl_learn_prioritized_draw, rl_learn_prioritized that the slots argument asks for anyway.  The arithmetic of the update is the D3QN instantiation's, instruction for instruction.
//
// Packing.  After the last step the workgroup rewrites `packed` from the final parameters: rl_policy.hip's pack_in_layer,
// pack_hidden_layer x 2, pack_head 128 -> 8 and pack_head 128 -> 1 at Layout.l1 / l2a / ha / l2b / hb, bit for bit.
#include "rl_learn_dev.h"

namespace {

constexpr int kDBlock = 512;
constexpr int kDRows = 64;                     // rows of a minibatch at most (rl_learner.batch)
constexpr int kAS = 160, kHS = 128;            // LDS row strides in floats (153 / 128 used; columns 153..159 of A are zero)
constexpr int kWTS = 36;                       // row stride of a forward weight tile [128][32]
constexpr int kWTFloats = 128 * kWTS;          // (>= the backward tile's 32 * 128)
constexpr int kErrLearnSlot = 6;               // error-flag code (include/reinlife_hip.h, rl_bind_error_flag)
constexpr int kLearnSite = RL_SITE_LEARN;
// state-dict-flat offsets of the dueling network (fc, adv_fc1, adv_fc2, value_fc1, value_fc2: weight then bias each)
constexpr int oW0 = 0, oB0 = 153 * 128, oWa1 = oB0 + 128, oBa1 = oWa1 + 128 * 128, oWa2 = oBa1 + 128, oBa2 = oWa2 + 8 * 128,
              oWv1 = oBa2 + 8, oBv1 = oWv1 + 128 * 128, oWv2 = oBv1 + 128, oBv2 = oWv2 + 128, kNParams = oBv2 + 1;
static_assert(kNParams == 53897, "the dueling network has 53,897 parameters");
constexpr int kNHead = 8 * 128 + 8 + 128 + 1;  // adv_fc2.weight, adv_fc2.bias | value_fc2.weight, value_fc2.bias
constexpr int kNFeat = 128 + 128 + 8 + 128 + 1;   // output features of the five layers (the packer's scales)

struct DuelBrain {
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

struct DuelPrio {                // the prioritised memory of a brain (k_learn_d3qn<true> only)
    float* priority;             // [ring capacity]
    float* prio_max;             // [1]
};

struct DuelArgs {
    DuelBrain b[RL_MAX_CAPTURE_BRAINS];
    DuelPrio p[RL_MAX_CAPTURE_BRAINS];
    const int32_t* slots;        // [n_learners][n_steps][batch] or null
    int32_t* err;
    uint64_t seed;
    int n_steps;
};

constexpr int kDLdsFloats = kDRows * kAS + 3 * kDRows * kHS + kWTFloats + kDRows * 8 + 6 * kDRows;
constexpr int kDLdsBytes = kDLdsFloats * 4;
static_assert(kDLdsBytes + 1024 <= 160 * 1024, "k_learn_d3qn's LDS map must fit a workgroup's 160 KiB");
static_assert(2 * kDRows * kHS >= kDRows * kAS, "HA + HV must hold the minibatch's observation rows");
static_assert(2 * kNFeat <= kWTFloats, "the packer's scales live in the weight tile");

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

// dW[o][k] = sum_rows D[row][o] * IN[row][k] (rows ascending) and Adam at once, for a layer of 128 outputs.  A work item is 4 outputs x 4
// consecutive k; consecutive threads take consecutive k groups.
template <int NIN, int DS, int INS>
__device__ __forceinline__ void duel_wgrad(const AdamStep& a, int off, const float* D, const float* IN, int tid)
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
                if (4 * kg + j < NIN) adam_update(a, off + (4 * og + i) * NIN + 4 * kg + j, acc[i][j]);
    }
}
template <int DS>
__device__ __forceinline__ void duel_bgrad(const AdamStep& a, int off, const float* D, int tid)
{
    if (tid < 128) {
        float g = 0.0f;
#pragma unroll 4
        for (int row = 0; row < kDRows; ++row) g += D[row * DS + tid];
        adam_update(a, off + tid, g);
    }
}

// the minibatch's rows of `src` (state or state_prime of the ring) -> X [64][160]; rows without a slot and columns >= 153 are zero
__device__ __forceinline__ void duel_stage_rows(const float* src, const int* row_slot, float* X, int tid)
{
    for (int i = tid; i < kDRows * kAS; i += kDBlock) {
        const int row = i / kAS, k = i - row * kAS, slot = row_slot[row];
        X[i] = (slot >= 0 && k < RL_OBS_DIM) ? src[(size_t)slot * RL_OBS_DIM + k] : 0.0f;
    }
}

// The network P on the rows in X: F, HA, HV as the file's header says, adv [64][8] and val [64] (no mean taken yet), row_sum[row] = the
// row's eight advantages added in action order.  Ends with a barrier.
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

// rl_policy_pack_weights(RL_D3QN, P) -> packed, by the whole workgroup.  sc / un: LDS [kNFeat] each, features of fc | adv_fc1 | adv_fc2 |
// value_fc1 | value_fc2.
__device__ __forceinline__ void duel_pack_hidden(const float* W, const float* bias, const float* sc, const float* un, float* dst, int tid)
{
    uint4* d = (uint4*)dst;
    for (int u = tid; u < 8 * 4 * 64; u += kDBlock) {                // pack_hidden_layer 128 -> 128: [s = 2t + c][t2][plane][lane]
        const int lane = u & 63, t2 = (u >> 6) & 3, s = u >> 8;
        const int o = 32 * t2 + (lane & 31);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = W[o * 128 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[o];
        uint4* q = d + ((s * 4 + t2) * kPlanes) * 64 + lane;
        learn_store_fragment(x, q, q + 64);
    }
    for (int ii = tid; ii < 256; ii += kDBlock) {                    // write_epilogue_consts
        const int r = ii & 15, th = ii >> 5;
        const int o = 32 * (th >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (th & 1);
        dst[frag_floats(8, 4) + ii] = (ii & 16) ? bias[o] : un[o];
    }
}
__device__ __forceinline__ void duel_pack_head(const float* W, const float* bias, int n_out, const float* sc, const float* un, float* dst, int tid)
{
    uint4* d = (uint4*)dst;
    for (int u = tid; u < 8 * 64; u += kDBlock) {                    // pack_head 128 -> n_out: [2t + c][plane][lane], rows >= n_out zero
        const int lane = u & 63, s = u >> 6;
        const int o = lane & 31;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = o < n_out ? W[o * 128 + learn_hidden_k(s >> 1, s & 1, e, lane)] * sc[o] : 0.0f;
        uint4* q = d + (s * kPlanes) * 64 + lane;
        learn_store_fragment(x, q, q + 64);
    }
    if (tid < 16) dst[head_consts_off(4) + tid] = tid < 8 ? (tid < n_out ? un[tid] : 1.0f) : (tid - 8 < n_out ? bias[tid - 8] : 0.0f);
}
__device__ __forceinline__ void duel_pack(const float* P, float* packed, float* sc, float* un, int tid)
{
    const Layout L = layout_of(RL_D3QN);
    if (tid < kNFeat) {   // feature_scales: 2^(kScaleExp - exponent(max |W[o][:]|))
        const int n_in = tid < 128 ? 153 : 128;
        const float* w = tid < 128 ? P + oW0 + tid * 153 : tid < 256 ? P + oWa1 + (tid - 128) * 128 : tid < 264 ? P + oWa2 + (tid - 256) * 128
                       : tid < 392 ? P + oWv1 + (tid - 264) * 128 : P + oWv2;
        float mx = 0.0f;
#pragma unroll 4
        for (int k = 0; k < n_in; ++k) mx = fmaxf(mx, fabsf(w[k]));
        row_scale(mx, sc[tid], un[tid]);
    }
    __syncthreads();
    uint4* d1 = (uint4*)(packed + L.l1);
    for (int u = tid; u < kInChunks * 4 * 64; u += kDBlock) {        // pack_in_layer: [c][t][plane][lane]
        const int lane = u & 63, t = (u >> 6) & 3, c = u >> 8;
        const int o = 32 * t + (lane & 31), k0 = 16 * c + 8 * (lane >> 5);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = k0 + e < 153 ? P[oW0 + o * 153 + k0 + e] * sc[o] : 0.0f;
        uint4* dst = d1 + ((c * 4 + t) * kPlanes) * 64 + lane;
        learn_store_fragment(x, dst, dst + 64);
    }
    for (int ii = tid; ii < 256; ii += kDBlock) {
        const int r = ii & 15, th = ii >> 5;
        const int o = 32 * (th >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (th & 1);
        packed[L.l1 + frag_floats(kInChunks, 4) + ii] = (ii & 16) ? P[oB0 + o] : un[o];
    }
    duel_pack_hidden(P + oWa1, P + oBa1, sc + 128, un + 128, packed + L.l2a, tid);
    duel_pack_head(P + oWa2, P + oBa2, 8, sc + 256, un + 256, packed + L.ha, tid);
    duel_pack_hidden(P + oWv1, P + oBv1, sc + 264, un + 264, packed + L.l2b, tid);
    duel_pack_head(P + oWv2, P + oBv2, 1, sc + 392, un + 392, packed + L.hb, tid);
}

template <bool PRIO>
__global__ __launch_bounds__(kDBlock) void k_learn_d3qn(const DuelArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float duel_lds[];
    float* xa = duel_lds;                           // A  [64][160]  (d_f [64][128] during the backward pass)
    float* fa = xa + kDRows * kAS;                  // F  [64][128]
    float* ha = fa + kDRows * kHS;                  // HA [64][128]  (da; with HV: the s rows again for fc's weight gradient)
    float* hv = ha + kDRows * kHS;                  // HV [64][128]  (dv)
    float* wt = hv + kDRows * kHS;                  // weight tile (the packer's sc / un)
    float* adv = wt + kWTFloats;                    // [64][8] advantages, then dL/dadv
    float* val = adv + kDRows * 8;                  // [64]
    float* row_sum = val + kDRows;                  // [64] a row's advantages added
    float* row_g = row_sum + kDRows;                // [64] dL/dq[a] = 2 td / batch
    float* row_r = row_g + kDRows;                  // [64] reward
    float* row_mask = row_r + kDRows;               // [64] 1 - done
    float* row_y = row_mask + kDRows;               // [64] max q', then td^2
    __shared__ int first_bad;
    __shared__ int row_slot[kDRows];
    __shared__ int row_a[kDRows];
    __shared__ float batch_mean, batch_G;

    const int tid = threadIdx.x, brain = blockIdx.x;
    const DuelBrain& B = A.b[brain];
    const int batch = B.batch, n_steps = A.n_steps;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    const long long calls = B.state[1];
    long long steps_taken = B.state[0];

    if (A.slots && size > B.min_size) {   // every slot of a call that trains is checked before anything is written: a bad one is a finding, never an address
        if (tid == 0) first_bad = 0x7fffffff;
        __syncthreads();
        const int32_t* sl = A.slots + (size_t)brain * n_steps * batch;
        for (int i = tid; i < n_steps * batch; i += kDBlock)
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
        // The buffers' addresses are re-read as opaque values in every step: otherwise the compiler hoists the per-lane addresses of every
        // parameter access of the step (hundreds of 64-bit values) in front of this loop and spills them.
        typedef float __attribute__((address_space(1))) gf;   // (global pointers stay global pointers through the asm)
        gf *gP = (gf*)B.params, *gT = (gf*)B.target, *gAM = (gf*)B.adam_m, *gAV = (gf*)B.adam_v, *gGR = (gf*)B.grad;
        const gf *gRS = (const gf*)B.r_state, *gRSP = (const gf*)B.r_state_prime;
        asm volatile("" : "+s"(gP), "+s"(gT), "+s"(gAM), "+s"(gAV), "+s"(gGR), "+s"(gRS), "+s"(gRSP));
        float *P = (float*)gP, *T = (float*)gT, *AM = (float*)gAM, *AV = (float*)gAV, *GR = (float*)gGR;
        const float *RS = (const float*)gRS, *RSP = (const float*)gRSP;
        // ---- the minibatch: rows >= batch are zero rows with a zero loss gradient, and stay out of the batch-wide mean ----
        if (tid < kDRows) {
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
        // ---- max_a q'_target(s'), q' = adv' + val' - M', M' the mean of the batch's adv' ----
        duel_stage_rows(RSP, row_slot, xa, tid);
        duel_network(T, xa, fa, ha, hv, wt, adv, val, row_sum, tid);
        if (tid == 0) {
            float sum = 0.0f;
            for (int j = 0; j < batch; ++j) sum += row_sum[j];
            batch_mean = sum / (float)(8 * batch);
        }
        __syncthreads();
        if (tid < kDRows) {
            const float m = batch_mean, v = val[tid];
            float mx = (adv[tid * 8] + v) - m;
            for (int a = 1; a < 8; ++a) mx = fmaxf(mx, (adv[tid * 8 + a] + v) - m);
            row_y[tid] = mx;
        }
        __syncthreads();
        // ---- q_eval(s), the MSE loss and dL/dq ----
        duel_stage_rows(RS, row_slot, xa, tid);
        duel_network(P, xa, fa, ha, hv, wt, adv, val, row_sum, tid);
        if (tid == 0) {
            float sum = 0.0f;
            for (int j = 0; j < batch; ++j) sum += row_sum[j];
            batch_mean = sum / (float)(8 * batch);
        }
        __syncthreads();
        if (tid < kDRows) {
            const float y = row_r[tid] + (B.gamma * row_mask[tid]) * row_y[tid];
            const float q = (adv[tid * 8 + row_a[tid]] + val[tid]) - batch_mean;
            const float td = q - y;
            const bool in = tid < batch;
            if (PRIO && in) A.p[brain].priority[row_slot[tid]] = fabsf(row_y[tid] - q);   // PERD3QN.py:110, from this step's pre-update parameters
            row_y[tid] = in ? td * td : 0.0f;
            row_g[tid] = in ? (2.0f * td) * inv_batch : 0.0f;
        }
        __syncthreads();
        if (tid == 0) {
            float sum = 0.0f, G = 0.0f;
            for (int j = 0; j < batch; ++j) { sum += row_y[j]; G += row_g[j]; }
            if (B.loss) B.loss[s] = sum * inv_batch;
            batch_G = G;
        }
        __syncthreads();
        {   // dL/dadv[i][a] = g_i [a = a_i] - G / (8 batch) on the batch's rows (the mean reaches every row and action), zero on padding rows
            const int row = tid >> 3, a = tid & 7;
            const float mean_term = batch_G / (float)(8 * batch);
            adv[tid] = row < batch ? (a == row_a[row] ? row_g[row] : 0.0f) - mean_term : 0.0f;
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
        // ---- gradients and Adam, parameter by parameter (nothing below reads a parameter of this network) ----
        const double t = (double)(steps_taken + 1);
        AdamStep ad;
        ad.p = P; ad.m = AM; ad.v = AV;
        ad.grad = GR ? GR + (size_t)s * kNParams : nullptr;
        ad.w1 = 1.0 - B.beta1; ad.w2 = 1.0 - B.beta2; ad.beta2 = B.beta2; ad.eps = B.eps_d;
        ad.bc2_sqrt = sqrt(1.0 - pow(B.beta2, t));
        ad.neg_step = -(B.lr / (1.0 - pow(B.beta1, t)));
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int idx = tid + kDBlock * p;
            if (idx < 1032) adam_update(ad, oWa2 + idx, head_g[p]);
            else if (idx < kNHead) adam_update(ad, oWv2 + idx - 1032, head_g[p]);
        }
        duel_wgrad<128, kHS, kHS>(ad, oWa1, ha, fa, tid);
        duel_bgrad<kHS>(ad, oBa1, ha, tid);
        duel_wgrad<128, kHS, kHS>(ad, oWv1, hv, fa, tid);
        duel_bgrad<kHS>(ad, oBv1, hv, tid);
        __syncthreads();   // HA and HV are free: the s rows come back from the ring
        duel_stage_rows(RS, row_slot, ha, tid);
        __syncthreads();
        duel_wgrad<153, kHS, kAS>(ad, oW0, xa, ha, tid);
        duel_bgrad<kHS>(ad, oB0, xa, tid);
        ++steps_taken;
        __syncthreads();   // the next step (and the packer) read the new parameters
    }
    if (B.sync_target)     // D3QN.py:125-126, on the caller's schedule
        for (int i = tid; i < kNParams; i += kDBlock) B.target[i] = B.params[i];
    if (tid == 0) { B.state[0] = steps_taken; B.state[1] = calls + 1; }
    if (PRIO && train && size > 0) {   // *prio_max = max(priority[0 .. size)) after a call that trained (a call below the size gate wrote no
                                       // priority and leaves the maximum alone): fmaxf is exact, so the order of the reduction does not matter
        const float* pr = A.p[brain].priority;
        float mx = 0.0f;      // (priorities are |.|: never below zero)
        for (long long i = tid; i < size; i += kDBlock) mx = fmaxf(mx, pr[i]);
        wt[tid] = mx;
        __syncthreads();
        for (int o = kDBlock / 2; o > 0; o >>= 1) {
            if (tid < o) wt[tid] = fmaxf(wt[tid], wt[tid + o]);
            __syncthreads();
        }
        if (tid == 0) *A.p[brain].prio_max = wt[0];
        __syncthreads();      // the packer's scales take the tile next
    }
    duel_pack(B.params, B.packed, wt, wt + kNFeat, tid);
}

}  // namespace

int rl_learn_dueling_supported_impl(int kind) { return kind == RL_D3QN ? 1 : 0; }

template <bool PRIO>
static int duel_launch(const char* who, rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, int n_steps,
                       const int32_t* slots, hipStream_t stream)
{
    DuelArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        DuelBrain& b = a.b[i];
        b.params = l.params; b.target = l.target; b.adam_m = l.adam_m; b.adam_v = l.adam_v;
        b.state = (long long*)l.state; b.packed = l.packed; b.loss = l.loss; b.grad = l.grad;
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done;
        b.r_count = r.count; b.r_capacity = r.capacity;
        b.lr = learn_decimal(l.lr); b.beta1 = learn_decimal(l.beta1); b.beta2 = learn_decimal(l.beta2);
        b.gamma = l.gamma; b.eps_d = learn_decimal(l.eps);
        b.batch = l.batch; b.min_size = l.min_size; b.sync_target = l.sync_target;
        if (PRIO) { a.p[i].priority = prios[i].priority; a.p[i].prio_max = prios[i].prio_max; }
    }
    a.slots = slots; a.err = h->err_flag; a.seed = h->cfg.seed; a.n_steps = n_steps;
    {   // the large dynamic-LDS window (158 KB): asked for at every call -- idempotent, host-only, and right on whatever device is current
        const hipError_t e = hipFuncSetAttribute((const void*)k_learn_d3qn<PRIO>, hipFuncAttributeMaxDynamicSharedMemorySize, kDLdsBytes);
        if (e != hipSuccess) { rl_set_error("%s: hipFuncSetAttribute(%d bytes of LDS) failed: %s", who, kDLdsBytes, hipGetErrorString(e)); return RL_E_LAUNCH; }
    }
    hipLaunchKernelGGL(k_learn_d3qn<PRIO>, dim3(n_learners), dim3(kDBlock), kDLdsBytes, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: kernel launch failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

int rl_learn_dueling_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
                            hipStream_t stream)
{
    return duel_launch<false>("rl_learn_dueling", h, learners, rings, nullptr, n_learners, n_steps, slots, stream);
}

int rl_learn_prioritized_supported_impl(int kind) { return kind == RL_PERD3QN ? 1 : 0; }

int rl_learn_prioritized_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, int n_steps,
                                const int32_t* slots, hipStream_t stream)
{
    return duel_launch<true>("rl_learn_prioritized", h, learners, rings, prios, n_learners, n_steps, slots, stream);
}
