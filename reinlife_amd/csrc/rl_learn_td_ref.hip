// rl_learn_td_ref.hip -- the prioritised memory of a PERDQN brain as the reference keeps it, for learn="reference": the sum tree itself, in
// float64 on the device, with the reference's rounding.  Memory.add for a group of new rows (rl_learn_td_tree_store), Memory.sample's
// stratified walk from uniforms the HOST has drawn (rl_learn_td_tree_sample) and train_model's update loop (rl_learn_td_tree_update).  The
// update of the network is rl_learn_td (rl_learn_td.hip), unchanged, on the slots the sample names.
//
// Reference (ReinLife/Models/PERDQN.py):
//   SumTree.update / _propagate  :209-215, 248-252  change = p - tree[idx]; tree[idx] = p; every proper ancestor += change, up to the root
//   SumTree._retrieve            :218-228           from node 0: left = 2 i + 1; no left child: a leaf; s <= tree[left] goes left, else
//                                                   s -= tree[left] and goes right
//   Memory.add                   :276-278           update(write + C - 1, p), write = rows stored so far % C.  append_sample hands it a
//                                                   float32 TORCH scalar: `p - tree[idx]` and `tree[parent] += change` are then torch
//                                                   operations in float32 (the float64 node is rounded to float32, added to, and the
//                                                   float32 sum stored back), unlike train_model's np.float32 errors, whose update
//                                                   runs in float64
//   Memory.sample                :280-298           segment = total / n; s_i = random.uniform(segment i, segment (i + 1))
//   train_model                  :175-177           for i in range(batch): memory.update(idxs[i], errors[i])
//
// Layout.  tree[2 C - 1] doubles: the leaf of memory index j at j + C - 1, the parent of i at (i - 1) / 2.  With L = i + 1 (the heap's
// 1-based numbering) a node's depth is floor(log2 L) and its ancestor k levels up is L >> k.  The leaves sit at one or two depths.
//
// The rounding order in parallel.  A sequence of updates (leaf_0, p_0), (leaf_1, p_1), ... is applied by the reference one after the
// other.  change_i = p_i - (the leaf's value just before update i) depends only on the earlier updates OF THAT LEAF: the value is p_j of
// the latest j < i with leaf_j = leaf_i, or what the tree held.  An inner node v receives v += change_i for exactly the updates i whose
// leaf lies below it, in the order of i: its final value is ((v + c_i1) + c_i2) + ... over ITS OWN subsequence i1 < i2 < ..., whatever
// the other nodes do meanwhile.  So k_tree_apply gives one thread to every (depth, update) pair; the thread of the FIRST update that touches
// a node at that depth owns the node: it reads the node once, walks the later updates in order adding the changes of those below the
// node, each add separately rounded (in double for an update batch, in float for a store group), and writes the node once.  The bits are the sequential reference's, in every run: no
// atomics, no order left to the scheduler.  Lists longer than kChunk updates are applied chunk after chunk by the same workgroup.
//
// All three entry points validate on the host and launch ONE kernel of one workgroup per learner; the formulas are in
// include/reinlife_hip.h.
#include "rl_common.h"

#include <math.h>

namespace {

constexpr int kApplyBlock = 256;
constexpr int kChunk = 256;              // the updates one pass stages in LDS
constexpr int kSampleBlock = 64;         // RL_LEARN_TD_TREE_BATCH_MAX
constexpr int kErrTree = 8;              // error-flag codes (include/reinlife_hip.h): a draw the reference would repeat ...
constexpr int kErrTreeIndex = 9;         // ... and an update entry outside the tree or the ring

struct ApplyBrain {
    double* tree;
    float* priority;
    const int32_t *idxs, *slots;         // update: the leaves and the ring slots their new priorities are read from; store: null
    long long capacity, ring_rows, first_row, n;
    float p_new;
};
struct ApplyArgs {
    ApplyBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* err;
};

// one workgroup per learner: the list of (leaf, value) -- a store group's rows or an update batch -- applied in list order
__global__ __launch_bounds__(kApplyBlock) void k_tree_apply(const ApplyArgs A)
{
    __shared__ int s_l1[kChunk];         // leaf + 1: the node in 1-based heap numbering (0: an entry that is skipped)
    __shared__ int s_depth[kChunk];      // floor(log2(leaf + 1))
    __shared__ double s_p[kChunk];       // the value the update writes
    __shared__ double s_change[kChunk];
    const ApplyBrain& B = A.b[blockIdx.x];
    const int tid = threadIdx.x;
    const long long C = B.capacity, R = B.ring_rows;
    const int n_nodes = (int)(2 * C - 1);
    const int depth_max = 31 - __clz(n_nodes);           // the depth of the last leaf: proper ancestors have depths 0 .. depth_max - 1

    for (long long base = 0; base < B.n; base += kChunk) {
        const int n = (int)(B.n - base < kChunk ? B.n - base : kChunk);
        if (tid < n) {
            int leaf; double p; bool ok = true;
            if (B.idxs) {                // train_model's loop: update(idxs[i], priority[slots[i]])
                leaf = B.idxs[base + tid];
                const int slot = B.slots[base + tid];
                ok = leaf >= C - 1 && leaf < n_nodes && slot >= 0 && slot < R;
                p = ok ? (double)B.priority[slot] : 0.0;
                if (!ok && A.err && atomicCAS(A.err, 0, kErrTreeIndex) == 0) { A.err[1] = (int)blockIdx.x; A.err[2] = (int)(base + tid); A.err[3] = leaf; }
            } else {                     // Memory.add: update(write + C - 1, p_new) for row first_row + base + tid
                const long long row = B.first_row + base + tid;
                leaf = (int)(row % C + C - 1);
                p = (double)B.p_new;
                B.priority[row % R] = B.p_new;
            }
            s_l1[tid] = ok ? leaf + 1 : 0;
            s_depth[tid] = ok ? 31 - __clz(leaf + 1) : 0;
            s_p[tid] = p;
        }
        __syncthreads();
        // the leaves: change_i = p_i - (the leaf's value in front of update i); the last update of a leaf writes it
        bool last = false;
        if (tid < n && s_l1[tid]) {
            const int l1 = s_l1[tid];
            int j = tid - 1;
            while (j >= 0 && s_l1[j] != l1) --j;
            const double old = j >= 0 ? s_p[j] : B.tree[l1 - 1];
            // (Memory.add hands update() a float32 torch scalar: its change and its sums are float32 operations, see the header)
            s_change[tid] = B.idxs ? __dsub_rn(s_p[tid], old) : (double)__fsub_rn((float)s_p[tid], (float)old);
            last = true;
            for (int k = tid + 1; k < n; ++k) last = last && s_l1[k] != l1;
        }
        __syncthreads();                 // every leaf has been read before one is written
        if (last) B.tree[s_l1[tid] - 1] = s_p[tid];
        // the inner nodes: one (depth, update) pair per thread and turn; the first update below a node owns it
        for (int w = tid; w < depth_max * n; w += kApplyBlock) {
            const int d = w / n, i = w - d * n;
            if (!s_l1[i] || s_depth[i] <= d) continue;
            const int node = s_l1[i] >> (s_depth[i] - d);
            bool owner = true;
            for (int j = 0; j < i && owner; ++j) owner = !(s_l1[j] && s_depth[j] > d && (s_l1[j] >> (s_depth[j] - d)) == node);
            if (!owner) continue;
            double v = B.tree[node - 1];
            for (int j = i; j < n; ++j)
                if (s_l1[j] && s_depth[j] > d && (s_l1[j] >> (s_depth[j] - d)) == node)
                    v = B.idxs ? __dadd_rn(v, s_change[j]) : (double)__fadd_rn((float)v, (float)s_change[j]);
            B.tree[node - 1] = v;
        }
        __syncthreads();                 // the next chunk reads what this one wrote, and overwrites the staging arrays
    }
}

struct SampleBrain {
    const double* tree;
    const double* u;
    int32_t *idxs, *slots;
    double *s, *leaves;                  // or null
    long long capacity, ring_rows, stored;
    int n;
};
struct SampleArgs {
    SampleBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* err;
};

__device__ inline int tree_slot(long long j, long long C, long long R, long long stored) { return (int)((j + C * ((stored - 1 - j) / C)) % R); }

// one workgroup of 64 threads per learner, one thread per draw
__global__ __launch_bounds__(kSampleBlock) void k_tree_sample(const SampleArgs A)
{
    __shared__ int s_bad;
    const SampleBrain& B = A.b[blockIdx.x];
    const int tid = threadIdx.x;
    const long long C = B.capacity, R = B.ring_rows, stored = B.stored;
    const int n_nodes = (int)(2 * C - 1);
    const long long filled = stored < C ? stored : C;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const double total = B.tree[0];
    int idx = 0;
    double s0 = 0.0;
    if (!(total > 0.0 && total < (double)INFINITY)) {
        if (tid == 0) {
            s_bad = 1;
            if (A.err && atomicCAS(A.err, 0, kErrTree) == 0) { A.err[1] = (int)blockIdx.x; A.err[2] = -1; A.err[3] = 0; }
        }
    } else if (tid < B.n) {
        const double segment = __ddiv_rn(total, (double)B.n);
        const double a = __dmul_rn(segment, (double)tid), b = __dmul_rn(segment, (double)(tid + 1));
        double s = s0 = __dadd_rn(a, __dmul_rn(__dsub_rn(b, a), B.u[tid]));      // random.uniform(a, b) = a + (b - a) * random()
        for (long long left = 1; left < n_nodes; left = 2ll * idx + 1) {         // at most 31 turns: idx at least doubles
            const double t = B.tree[left];
            if (s <= t) idx = (int)left;
            else { s = __dsub_rn(s, t); idx = (int)left + 1; }
        }
        const long long j = idx - (C - 1);
        if (j >= filled) {               // a leaf no row has reached: the reference would draw again
            s_bad = 1;
            if (A.err && atomicCAS(A.err, 0, kErrTree) == 0) { A.err[1] = (int)blockIdx.x; A.err[2] = tid; A.err[3] = (int)j; }
        }
    }
    __syncthreads();
    if (tid >= B.n) return;
    if (s_bad) {                         // every draw of the learner names memory index 0
        B.idxs[tid] = (int32_t)(C - 1);
        B.slots[tid] = tree_slot(0, C, R, stored);
        return;
    }
    B.idxs[tid] = idx;
    B.slots[tid] = tree_slot(idx - (C - 1), C, R, stored);
    if (B.s) B.s[tid] = s0;
    if (B.leaves) B.leaves[tid] = B.tree[idx];
}

int device_of(const void* p)
{
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged ? a.device : -1;
}
struct Guard {   // the buffers' device is current for the launch (rl_capi.hip's DeviceGuard)
    int prev = -1;
    explicit Guard(int dev)
    {
        int cur = -1;
        if (dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~Guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// what the three entry points ask of their common arguments
int check_common(const char* who, rl_world* h, const rl_learner* learners, const rl_tdprio* tds, const void* per_learner, int n_learners)
{
    if (!h) { rl_set_error("%s: null handle", who); return RL_E_INVALID; }
    if (!learners || !tds || !per_learner) { rl_set_error("%s: null learners / tds / per-learner arguments", who); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("%s: n_learners must be in [1,%d] (got %d)", who, RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i)
        if (learners[i].kind != RL_PERDQN) { rl_set_error("%s: learner %d has brain kind %d; this entry point serves RL_PERDQN (4) only", who, i, learners[i].kind); return RL_E_UNSUPPORTED; }
    return RL_OK;
}
int check_tree(const char* who, int i, const void* tree, long long capacity, long long ring_rows)
{
    if (!tree) { rl_set_error("%s: learner %d: tree must not be null", who, i); return RL_E_INVALID; }
    if (capacity < 2 || capacity > (1ll << 30)) {
        rl_set_error("%s: learner %d: capacity must be in [2, 2^30] (got %lld): a tree of one leaf has no root to propagate to (the reference's "
                     "_propagate never ends there), and tree indices are int32", who, i, capacity);
        return RL_E_INVALID;
    }
    if (ring_rows < capacity || ring_rows > 0x7fffffffll) { rl_set_error("%s: learner %d: ring_rows must be in [capacity, 2^31) (got %lld, capacity %lld)", who, i, ring_rows, capacity); return RL_E_INVALID; }
    return RL_OK;
}
int launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

}  // namespace

extern "C" {

int rl_learn_td_tree_store(rl_world* h, const rl_learner* learners, const rl_tdprio* tds, const rl_td_tree_store* groups, int n_learners,
                           void* stream)
{
    const char* who = "rl_learn_td_tree_store";
    if (int rc = check_common(who, h, learners, tds, groups, n_learners)) return rc;
    ApplyArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_td_tree_store& g = groups[i];
        if (int rc = check_tree(who, i, g.tree, g.capacity, g.ring_rows)) return rc;
        if (!tds[i].priority) { rl_set_error("%s: td %d: priority must not be null", who, i); return RL_E_INVALID; }
        if (g.first_row < 0) { rl_set_error("%s: learner %d: first_row must be >= 0 (got %lld)", who, i, g.first_row); return RL_E_INVALID; }
        if (g.n_rows < 1 || g.n_rows > g.ring_rows - g.capacity) {
            rl_set_error("%s: learner %d: n_rows must be in [1, ring_rows - capacity] = [1, %lld] (got %lld): a longer group would overwrite the "
                         "ring slots of rows the memory still holds", who, i, g.ring_rows - g.capacity, g.n_rows);
            return RL_E_INVALID;
        }
        a.b[i] = ApplyBrain{g.tree, tds[i].priority, nullptr, nullptr, g.capacity, g.ring_rows, g.first_row, g.n_rows, tds[i].p_new};
    }
    a.err = h->err_flag;
    Guard guard(device_of(groups[0].tree));
    hipLaunchKernelGGL(k_tree_apply, dim3(n_learners), dim3(kApplyBlock), 0, (hipStream_t)stream, a);
    return launched(who);
}

int rl_learn_td_tree_sample(rl_world* h, const rl_learner* learners, const rl_tdprio* tds, const rl_td_tree_sample* draws, int n_learners,
                            void* stream)
{
    const char* who = "rl_learn_td_tree_sample";
    if (int rc = check_common(who, h, learners, tds, draws, n_learners)) return rc;
    SampleArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_td_tree_sample& d = draws[i];
        if (int rc = check_tree(who, i, d.tree, d.capacity, d.ring_rows)) return rc;
        if (d.stored < 1) { rl_set_error("%s: learner %d: stored must be >= 1 (got %lld): an empty memory has no row to draw", who, i, d.stored); return RL_E_INVALID; }
        if (d.n < 1 || d.n > RL_LEARN_TD_TREE_BATCH_MAX) { rl_set_error("%s: learner %d: n must be in [1,%d] (got %d)", who, i, RL_LEARN_TD_TREE_BATCH_MAX, d.n); return RL_E_INVALID; }
        if (!d.u || !d.idxs || !d.slots) { rl_set_error("%s: learner %d: u / idxs / slots must not be null", who, i); return RL_E_INVALID; }
        a.b[i] = SampleBrain{d.tree, d.u, d.idxs, d.slots, d.s, d.leaves, d.capacity, d.ring_rows, d.stored, d.n};
    }
    a.err = h->err_flag;
    Guard guard(device_of(draws[0].tree));
    hipLaunchKernelGGL(k_tree_sample, dim3(n_learners), dim3(kSampleBlock), 0, (hipStream_t)stream, a);
    return launched(who);
}

int rl_learn_td_tree_update(rl_world* h, const rl_learner* learners, const rl_tdprio* tds, const rl_td_tree_update* batches, int n_learners,
                            void* stream)
{
    const char* who = "rl_learn_td_tree_update";
    if (int rc = check_common(who, h, learners, tds, batches, n_learners)) return rc;
    ApplyArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_td_tree_update& b = batches[i];
        if (int rc = check_tree(who, i, b.tree, b.capacity, b.ring_rows)) return rc;
        if (!tds[i].priority) { rl_set_error("%s: td %d: priority must not be null", who, i); return RL_E_INVALID; }
        if (b.n < 1 || b.n > RL_LEARN_TD_TREE_BATCH_MAX) { rl_set_error("%s: learner %d: n must be in [1,%d] (got %d)", who, i, RL_LEARN_TD_TREE_BATCH_MAX, b.n); return RL_E_INVALID; }
        if (!b.idxs || !b.slots) { rl_set_error("%s: learner %d: idxs / slots must not be null", who, i); return RL_E_INVALID; }
        a.b[i] = ApplyBrain{b.tree, tds[i].priority, b.idxs, b.slots, b.capacity, b.ring_rows, 0, b.n, 0.0f};
    }
    a.err = h->err_flag;
    Guard guard(device_of(batches[0].tree));
    hipLaunchKernelGGL(k_tree_apply, dim3(n_learners), dim3(kApplyBlock), 0, (hipStream_t)stream, a);
    return launched(who);
}

}  // extern "C"
