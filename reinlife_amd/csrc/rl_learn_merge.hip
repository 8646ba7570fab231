// rl_learn_merge.hip -- what several ranks need to train together (include/reinlife_hip.h, "learning on several ranks"): a learner's
// state as one flat row (k_merge_export), the deterministic mean of the rows of all ranks back into the learner (k_merge_mean), and
// rl_policy.hip's host packer on the device for every brain kind (k_pack_device), which also serves rl_policy_pack_device and the end
// of an rl_learn_wide call.
// This build's own: the reference has no multi-process training.  No matrix work, no LDS tiles: three memory-bound kernels.
//
// Row segment of one learner (rl_learn_merge_floats = 3 n_params + 2 floats): params | adam_m | adam_v | state[0] as two 32-bit words,
// low then high.  3 * 53,897 is odd, so a segment's step words are NOT 8-byte aligned: every access to a row is a 4-byte one.
//
// k_merge_export   grid (ceil(longest segment / 256), n_learners): thread e of learner i copies float e of its segment -- consecutive
//                  lanes, consecutive addresses on both sides.
// k_merge_mean     grid (ceil(most parameters / 256), n_learners).  A workgroup first reads its learner's step words of the n_ranks rows
//                  (<= 64 pairs, one per thread), takes their maximum and the 64-bit mask of the ranks that hold it: the participants.
//                  Then one thread per element: for params, adam_m and adam_v the participants' values are summed in rank order in double,
//                  divided by their number in double and rounded to float once -- the same bits on every rank and in every run.  Lane l
//                  reads rows[r][seg + e0 + l]: coalesced per rank.  The rows are only read and the learner's buffers only written, so a
//                  row may not alias a learner's buffer, and the kernel needs no ordering between its workgroups.  state[0] <- the maximum
//                  (one thread per learner); target <- merged params where sync_target is set.  The sums start from -0.0, so a single
//                  participant gives ((-0.0) + x) / 1.0 = x, the sign of a zero included: n_ranks = 1 is the identity.
// k_pack_device    grid (17, n_learners): a workgroup packs one output tile (32 features) of one layer -- at most 17 tiles (PPO: 8 + 8 + 1).
//                  It computes the tile's 32 row scales (8 threads per feature, fmaxf in any order is exact), then every fragment of the
//                  tile and the tile's epilogue constants.  One function over (n_in, n_out, rne) for the three layer shapes of
//                  rl_policy.hip: pack_in_layer, pack_hidden_layer, pack_head.  Bit for bit the host packer: the scale is a power of two
//                  (the product is exact), the f16 split is rl_learn_dev.h's integer code.
#include "rl_learn_dev.h"

int64_t rl_policy_n_params_impl(int);   // rl_policy.hip

namespace {

constexpr int kMBlock = 256;
constexpr int kMaxRanks = 64;
constexpr int kMaxLayers = 5;      // the dueling kinds: fc, adv_fc1, adv_fc2, value_fc1, value_fc2
constexpr int kMaxTiles = 17;      // PPO: 8 + 8 + 1 output tiles

struct MergeBrain {
    float *params, *target, *adam_m, *adam_v;
    long long* state;
    long long seg;                 // first float of the learner's segment within a row
    int n_params, sync_target;
};
struct MergeArgs {
    MergeBrain b[RL_MAX_CAPTURE_BRAINS];
    const float* rows;             // merge: [n_ranks][stride]
    float* row;                    // export: one row
    long long stride;
    int n_ranks;
};

struct PackBrain {
    const float* params;
    float* packed;
    int kind;
    const long long* bad;          // null, or one device word: non-zero leaves `packed` as it is (rl_learn_wide's learner with a bad slot)
};
struct PackArgs {
    PackBrain b[RL_MAX_CAPTURE_BRAINS];
};

enum { kLayerIn = 0, kLayerHidden = 1, kLayerHead = 2 };
struct PackLayer {
    int type, n_in, n_out;
    int w, b;                      // state-dict-flat offsets of the weight matrix [n_out][n_in] and the bias
    long long dst;                 // offset of the layer in `packed`
};

// the layers of a kind in rl_policy_pack_impl's order; returns their number
__host__ __device__ inline int pack_layers_of(int kind, PackLayer (&ly)[kMaxLayers])
{
    const Layout L = layout_of(kind);
    int p = 0, n = 0;
    auto add = [&](int type, int n_in, int n_out, long long dst) {
        ly[n++] = PackLayer{type, n_in, n_out, p, p + n_in * n_out, dst};
        p += n_in * n_out + n_out;
    };
    if (kind == RL_DQN) {
        add(kLayerIn, 153, 128, L.l1); add(kLayerHidden, 128, 64, L.l2a); add(kLayerHead, 64, 8, L.ha);
    } else if (kind == RL_D3QN || kind == RL_PERD3QN) {
        add(kLayerIn, 153, 128, L.l1); add(kLayerHidden, 128, 128, L.l2a); add(kLayerHead, 128, 8, L.ha);
        add(kLayerHidden, 128, 128, L.l2b); add(kLayerHead, 128, 1, L.hb);
    } else if (kind == RL_PPO) {
        add(kLayerIn, 153, 256, L.l1); add(kLayerHidden, 256, 256, L.l2a); add(kLayerHead, 256, 8, L.ha);   // (fc_v is not packed)
    } else {
        add(kLayerIn, 153, 64, L.l1); add(kLayerHidden, 64, 64, L.l2a); add(kLayerHead, 64, 8, L.ha);
    }
    return n;
}

__global__ __launch_bounds__(kMBlock) void k_merge_export(const MergeArgs A)
{
    const MergeBrain& B = A.b[blockIdx.y];
    const int e = blockIdx.x * kMBlock + threadIdx.x;
    const int n = B.n_params;
    if (e >= 3 * n + 2) return;
    float v;
    if (e < n) v = B.params[e];
    else if (e < 2 * n) v = B.adam_m[e - n];
    else if (e < 3 * n) v = B.adam_v[e - 2 * n];
    else {
        const unsigned long long s = (unsigned long long)B.state[0];
        v = __uint_as_float(e == 3 * n ? (uint32_t)s : (uint32_t)(s >> 32));
    }
    A.row[B.seg + e] = v;
}

__global__ __launch_bounds__(kMBlock) void k_merge_mean(const MergeArgs A)
{
    __shared__ unsigned long long s_steps[kMaxRanks];
    __shared__ unsigned long long s_mask;
    const MergeBrain& B = A.b[blockIdx.y];
    const int n = B.n_params, tid = threadIdx.x;
    if (blockIdx.x * kMBlock >= n) return;   // (the whole workgroup: the grid is sized for the learner with the most parameters)
    const float* seg = A.rows + B.seg;
    if (tid < A.n_ranks) {
        const float* w = seg + (long long)tid * A.stride + 3 * (long long)n;
        s_steps[tid] = (unsigned long long)__float_as_uint(w[0]) | ((unsigned long long)__float_as_uint(w[1]) << 32);
    }
    __syncthreads();
    if (tid == 0) {
        long long mx = (long long)s_steps[0];
        for (int r = 1; r < A.n_ranks; ++r) mx = (long long)s_steps[r] > mx ? (long long)s_steps[r] : mx;
        unsigned long long mask = 0;
        for (int r = 0; r < A.n_ranks; ++r) mask |= (unsigned long long)((long long)s_steps[r] == mx) << r;
        s_mask = mask;
        if (blockIdx.x == 0) B.state[0] = mx;
    }
    __syncthreads();
    const unsigned long long mask = s_mask;
    const double count = (double)__popcll(mask);
    const int e = blockIdx.x * kMBlock + tid;
    if (e >= n) return;
    double sp = -0.0, sm = -0.0, sv = -0.0;   // -0.0 is the additive identity: (-0.0) + x = x for every x, a lone -0.0 included
#pragma unroll 4
    for (int r = 0; r < A.n_ranks; ++r) {
        const float* row = seg + (long long)r * A.stride;
        const float p = row[e], m = row[n + e], v = row[2 * (long long)n + e];   // (loaded whether the rank takes part or not: no branch in front of a load)
        if ((mask >> r) & 1ull) { sp += (double)p; sm += (double)m; sv += (double)v; }
    }
    const float mp = (float)(sp / count);
    B.params[e] = mp;
    B.adam_m[e] = (float)(sm / count);
    B.adam_v[e] = (float)(sv / count);
    if (B.sync_target && B.target) B.target[e] = mp;
}

// One output tile of one layer, by the whole workgroup.  sc / un: LDS [32].
//   in      fragment [c][t][plane][lane], o = 32 t + (lane & 31), k = 16 c + 8 (lane >> 5) + e, zero for k >= 153
//   hidden  fragment [s = 2 t + c][t2][plane][lane], o = 32 t2 + (lane & 31), k = learn_hidden_k(t, c, e, lane)
//   head    fragment [s][plane][lane], o = lane & 31, rows >= n_out zero; then unscale[8] (1 for unused outputs), bias[8] (0 for unused)
__device__ __forceinline__ void pack_tile(const PackLayer& ly, int t2, bool rne, const float* P, float* packed, float* sc, float* un, int tid)
{
    const float* W = P + ly.w;
    const float* bias = P + ly.b;
    const int n_in = ly.n_in, n_out = ly.n_out;
    {   // feature_scales: 2^(kScaleExp - exponent(max |W[o][:]|)) of the tile's 32 features, 8 threads per feature
        const int f = tid >> 3, o = 32 * t2 + f;
        float mx = 0.0f;
        if (o < n_out)
            for (int k = tid & 7; k < n_in; k += 8) mx = fmaxf(mx, fabsf(W[(size_t)o * n_in + k]));
        mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4));
        if ((tid & 7) == 0) row_scale(mx, sc[f], un[f]);
    }
    __syncthreads();
    float* dst = packed + ly.dst;
    uint4* d = (uint4*)dst;
    const int chunks = ly.type == kLayerIn ? kInChunks : n_in / 16;   // fragments of the tile along k (hidden / head: s = 2 t + c)
    const int tout = ly.type == kLayerHead ? 1 : n_out / 32;
    for (int u = tid; u < chunks * 64; u += kMBlock) {
        const int lane = u & 63, s = u >> 6;
        const int f = lane & 31, o = 32 * t2 + f;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = ly.type == kLayerIn ? 16 * s + 8 * (lane >> 5) + e : learn_hidden_k(s >> 1, s & 1, e, lane);
            x[e] = (o < n_out && k < n_in) ? W[(size_t)o * n_in + k] * sc[f] : 0.0f;
        }
        uint4* hi = d + ((size_t)(s * tout + t2) * kPlanes) * 64 + lane;
        if (rne) learn_store_fragment_rne(x, hi, hi + 64);
        else learn_store_fragment(x, hi, hi + 64);
    }
    if (ly.type == kLayerHead) {
        if (tid < 16) dst[head_consts_off(n_in / 32) + tid] = tid < 8 ? (tid < n_out ? un[tid] : 1.0f) : (tid - 8 < n_out ? bias[tid - 8] : 0.0f);
    } else if (tid < 64) {
        // write_epilogue_consts: per lane half h [unscale 16 | bias 16], feature 32 t2 + (r&3) + 8(r>>2) + 4h
        const int r = tid & 15, h = tid >> 5;
        const int f = (r & 3) + 8 * (r >> 2) + 4 * h;
        dst[frag_floats(chunks, tout) + (size_t)t2 * 64 + tid] = (tid & 16) ? bias[32 * t2 + f] : un[f];
    }
}

__global__ __launch_bounds__(kMBlock) void k_pack_device(const PackArgs A)
{
    __shared__ float sc[32], un[32];
    const PackBrain& B = A.b[blockIdx.y];
    if (B.bad && *B.bad) return;   // (the whole workgroup)
    PackLayer ly[kMaxLayers];
    const int n_layers = pack_layers_of(B.kind, ly);
    int tile = blockIdx.x;
#pragma unroll
    for (int i = 0; i < kMaxLayers; ++i) {
        if (i >= n_layers) return;   // (wave-uniform: the tile index is the workgroup's)
        const int tiles = ly[i].type == kLayerHead ? 1 : ly[i].n_out / 32;
        if (tile < tiles) {
            pack_tile(ly[i], tile, B.kind == RL_PERDQN, B.params, B.packed, sc, un, threadIdx.x);
            return;
        }
        tile -= tiles;
    }
}

int launch_pack(const char* who, const PackArgs& a, int n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_pack_device, dim3(kMaxTiles, n), dim3(kMBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: launch of the pack kernel failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

// segments laid end to end in learner order; returns the floats of a whole row
long long fill_merge_args(MergeArgs& a, const rl_learner* learners, int n_learners, int& max_params)
{
    long long seg = 0;
    max_params = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        MergeBrain& b = a.b[i];
        b.params = l.params; b.target = l.target; b.adam_m = l.adam_m; b.adam_v = l.adam_v; b.state = (long long*)l.state;
        b.n_params = (int)rl_policy_n_params_impl(l.kind); b.sync_target = l.sync_target; b.seg = seg;
        seg += 3 * (long long)b.n_params + 2;
        max_params = b.n_params > max_params ? b.n_params : max_params;
    }
    return seg;
}

}  // namespace

int64_t rl_learn_merge_floats_impl(int kind)
{
    const int64_t n = rl_policy_n_params_impl(kind);
    return n < 0 ? -1 : 3 * n + 2;
}

int rl_learn_export_launch(rl_world*, const rl_learner* learners, int n_learners, float* row, hipStream_t stream)
{
    MergeArgs a{};
    int max_params;
    fill_merge_args(a, learners, n_learners, max_params);
    a.row = row;
    hipLaunchKernelGGL(k_merge_export, dim3((3 * max_params + 2 + kMBlock - 1) / kMBlock, n_learners), dim3(kMBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_export: launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

int rl_learn_merge_launch(rl_world*, const rl_learner* learners, int n_learners, const float* rows, int n_ranks, int64_t row_stride_floats,
                          hipStream_t stream)
{
    MergeArgs a{};
    int max_params;
    fill_merge_args(a, learners, n_learners, max_params);
    a.rows = rows; a.stride = row_stride_floats; a.n_ranks = n_ranks;
    hipLaunchKernelGGL(k_merge_mean, dim3((max_params + kMBlock - 1) / kMBlock, n_learners), dim3(kMBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_merge: launch of the mean kernel failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    PackArgs p{};
    for (int i = 0; i < n_learners; ++i) p.b[i] = PackBrain{learners[i].params, learners[i].packed, learners[i].kind, nullptr};
    return launch_pack("rl_learn_merge", p, n_learners, stream);
}

// the packer at the end of an rl_learn_wide call: bad[i] is learner i's "bad slot" word, written earlier on the same stream
int rl_learn_wide_pack_launch(const rl_learner* learners, int n_learners, const long long* const* bad, hipStream_t stream)
{
    PackArgs p{};
    for (int i = 0; i < n_learners; ++i) p.b[i] = PackBrain{learners[i].params, learners[i].packed, learners[i].kind, bad[i]};
    return launch_pack("rl_learn_wide", p, n_learners, stream);
}

int rl_policy_pack_device_launch(int kind, const float* params, float* packed, hipStream_t stream)
{
    PackArgs p{};
    p.b[0] = PackBrain{params, packed, kind, nullptr};
    return launch_pack("rl_policy_pack_device", p, 1, stream);
}
