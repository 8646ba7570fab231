// rl_learn_prio_ref.hip -- the prioritised memory of a PERD3QN brain as the reference keeps it, for learn="reference": store()'s rule for
// new rows (rl_learn_prioritized_store_ref) and sample()'s np.random.choice from uniforms the HOST has drawn (rl_learn_prioritized_choice).
// The priorities never leave the device; the update itself is rl_learn_prioritized (rl_learn_dueling.hip), on the slots the choice names.
//
// Reference (ReinLife/Models/PERD3QN.py):
//   PrioritizedReplayBuffer.store    :143-155  a new row gets np.max(priorities) as of that store, 1.0 into an empty memory
//   PrioritizedReplayBuffer.sample   :157-165  probs = priorities[:len] ** alpha; probs /= probs.sum(); np.random.choice(len, batch, p=probs)
// np.random.choice(n, size, p=p) draws `size` doubles of random_sample() and answers cdf.searchsorted(u, side="right") with
// cdf = p.cumsum() (in float64) / cdf[-1]: the host makes those draws from np.random without seeing a priority, the device walks the cdf.
//
// Rows and slots.  Row a (numbered from 0 in storage order) sits in ring slot a % R and at the reference's memory index a % C, R >= C the
// rows the ring holds.  `priority` is indexed by ring slot.  With `stored` rows stored, memory index i < n = min(stored, C) holds row
// a_i = i + C * ((stored - 1 - i) / C): the latest row whose index is i.
//
// Both entry points validate on the host and launch ONE kernel of one workgroup per learner; the formulas are in include/reinlife_hip.h.
#include "rl_common.h"

#include <math.h>

namespace {

constexpr int kStoreBlock = 256;
constexpr int kChoiceBlock = 1024;       // the chunks of the two sums: memory indices [t L, (t + 1) L), L = ceil(n / 1024), t = 0 .. 1023
constexpr int kErrNoDistribution = 7;    // error-flag code (include/reinlife_hip.h)
constexpr long long kNoRow = 0x7fffffffffffffffll;

struct StoreBrain {
    float* priority;
    long long capacity, ring_rows, first_row, n_rows;
};
struct StoreArgs {
    StoreBrain b[RL_MAX_CAPTURE_BRAINS];
};

// one workgroup per learner: M = the maximum over the live window in front of row a, then priority[(a + j) % R] = M for j < m
__global__ __launch_bounds__(kStoreBlock) void k_prio_store_ref(const StoreArgs A)
{
    __shared__ float s_max[kStoreBlock];
    __shared__ long long s_nan[kStoreBlock];
    const StoreBrain& B = A.b[blockIdx.x];
    const int tid = threadIdx.x;
    const long long a = B.first_row, m = B.n_rows, C = B.capacity, R = B.ring_rows;
    float M = 1.0f;                      // PERD3QN.py:147: the first row of an empty memory
    if (a > 0) {
        float mx = -INFINITY;
        long long nan_row = kNoRow;      // the earliest row of the window that holds a NaN: np.max answers a NaN then
        for (long long r = (a > C ? a - C : 0) + tid; r < a; r += kStoreBlock) {
            const float p = B.priority[r % R];
            if (p != p) nan_row = r < nan_row ? r : nan_row;
            else mx = fmaxf(mx, p);
        }
        s_max[tid] = mx; s_nan[tid] = nan_row;
        __syncthreads();
        for (int o = kStoreBlock / 2; o > 0; o >>= 1) {
            if (tid < o) {
                s_max[tid] = fmaxf(s_max[tid], s_max[tid + o]);
                s_nan[tid] = s_nan[tid + o] < s_nan[tid] ? s_nan[tid + o] : s_nan[tid];
            }
            __syncthreads();
        }
        mx = s_max[0];
        if (a < C) mx = fmaxf(mx, 0.0f);                     // the zeros of the memory indices no row has reached yet
        M = s_nan[0] != kNoRow ? B.priority[s_nan[0] % R] : mx;
    }
    __syncthreads();                     // (window and group share no slot, m <= R - C; the barrier keeps that from being load-bearing)
    for (long long j = tid; j < m; j += kStoreBlock) B.priority[(a + j) % R] = M;
}

struct ChoiceBrain {
    const float* priority;
    const double* u;
    int32_t *indices, *slots;
    double* bracket;                     // [batch][2] or null
    double* cdf;                         // work: [capacity] doubles ...
    float* w;                            // ... then [capacity] floats
    long long capacity, ring_rows, stored;
    double alpha;
    int batch;
};
struct ChoiceArgs {
    ChoiceBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* err;
};

__device__ inline long long choice_row(long long i, long long C, long long stored) { return i + C * ((stored - 1 - i) / C); }

// one workgroup per learner: weights, their sum, the probabilities' running sum, the normalised cdf, then one binary search per draw
__global__ __launch_bounds__(kChoiceBlock) void k_prio_choice(const ChoiceArgs A)
{
    __shared__ double part[kChoiceBlock];
    __shared__ double s_total;
    __shared__ float s_sum;
    const ChoiceBrain& B = A.b[blockIdx.x];
    const int tid = threadIdx.x;
    const long long C = B.capacity, R = B.ring_rows, stored = B.stored;
    const long long n = stored < C ? stored : C;
    const long long L = (n + kChoiceBlock - 1) / kChoiceBlock;
    const long long i0 = (long long)tid * L < n ? (long long)tid * L : n;
    const long long i1 = i0 + L < n ? i0 + L : n;

    double s = 0.0;                      // w_i = (float)pow((double)p_i, alpha); chunk sums in double, in index order
    for (long long i = i0; i < i1; ++i) {
        const float wi = (float)pow((double)B.priority[choice_row(i, C, stored) % R], B.alpha);
        B.w[i] = wi;
        s += (double)wi;
    }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {                      // S = (float)(((c_0 + c_1) + c_2) + ...)
        double t = 0.0;
        for (int k = 0; k < kChoiceBlock; ++k) t += part[k];
        s_sum = (float)t;
    }
    __syncthreads();
    const float S = s_sum;

    double run = 0.0;                    // q_i = w_i / S in float; the running sum of (double)q_i inside the chunk
    for (long long i = i0; i < i1; ++i) {
        run += (double)(B.w[i] / S);
        B.cdf[i] = run;
    }
    part[tid] = run;                     // (thread 0 has read every part[] before the barrier above)
    __syncthreads();
    if (tid == 0) {                      // o_t = ((c_0 + c_1) + ...) + c_{t-1}; the total is the unnormalised cdf of the last index
        double t = 0.0;
        for (int k = 0; k < kChoiceBlock; ++k) { const double c = part[k]; part[k] = t; t += c; }
        s_total = t;
    }
    __syncthreads();
    const double total = s_total, off = part[tid];

    if (!(total > 0.0 && total < (double)INFINITY)) {   // all weights zero, a NaN, a negative priority, an overflow: np.random.choice raises
        if (tid == 0 && A.err && atomicCAS(A.err, 0, kErrNoDistribution) == 0) { A.err[1] = (int)blockIdx.x; A.err[2] = (int)n; A.err[3] = 0; }
        if (tid < B.batch) { B.indices[tid] = 0; B.slots[tid] = (int32_t)(choice_row(0, C, stored) % R); }
        return;                          // (uniform)
    }
    for (long long i = i0; i < i1; ++i) B.cdf[i] = (off + B.cdf[i]) / total;
    __syncthreads();

    if (tid < B.batch) {                 // idx = #{i : cdf_i <= u}: searchsorted(side="right") on a nondecreasing cdf that ends in 1.0
        const double u = B.u[tid];
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (B.cdf[mid] <= u) lo = mid + 1; else hi = mid;
        }
        const long long idx = lo < n ? lo : n - 1;   // (a u >= 1 is no draw of random_sample; it names the last row)
        B.indices[tid] = (int32_t)idx;
        B.slots[tid] = (int32_t)(choice_row(idx, C, stored) % R);
        if (B.bracket) { B.bracket[2 * tid] = idx > 0 ? B.cdf[idx - 1] : 0.0; B.bracket[2 * tid + 1] = B.cdf[idx]; }
    }
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

// what both entry points ask of their common arguments
int check_common(const char* who, rl_world* h, const rl_learner* learners, const rl_prio* prios, const void* per_learner, int n_learners)
{
    if (!h) { rl_set_error("%s: null handle", who); return RL_E_INVALID; }
    if (!learners || !prios || !per_learner) { rl_set_error("%s: null learners / prios / per-learner arguments", who); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("%s: n_learners must be in [1,%d] (got %d)", who, RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i) {
        if (learners[i].kind != RL_PERD3QN) { rl_set_error("%s: learner %d has brain kind %d; this entry point serves RL_PERD3QN (2) only", who, i, learners[i].kind); return RL_E_UNSUPPORTED; }
        if (!prios[i].priority) { rl_set_error("%s: prio %d: priority must not be null", who, i); return RL_E_INVALID; }
    }
    return RL_OK;
}
int check_rows(const char* who, int i, long long capacity, long long ring_rows)
{
    if (capacity < 1 || capacity > 0x7fffffffll) { rl_set_error("%s: learner %d: capacity must be in [1, 2^31) (got %lld): slots and indices are int32", who, i, capacity); return RL_E_INVALID; }
    if (ring_rows < capacity || ring_rows > 0x7fffffffll) { rl_set_error("%s: learner %d: ring_rows must be in [capacity, 2^31) (got %lld, capacity %lld)", who, i, ring_rows, capacity); return RL_E_INVALID; }
    return RL_OK;
}

}  // namespace

extern "C" {

int rl_learn_prioritized_store_ref(rl_world* h, const rl_learner* learners, const rl_prio* prios, const rl_prio_store* groups, int n_learners,
                                   void* stream)
{
    const char* who = "rl_learn_prioritized_store_ref";
    if (int rc = check_common(who, h, learners, prios, groups, n_learners)) return rc;
    StoreArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_prio_store& g = groups[i];
        if (int rc = check_rows(who, i, g.capacity, g.ring_rows)) return rc;
        if (g.first_row < 0) { rl_set_error("%s: learner %d: first_row must be >= 0 (got %lld)", who, i, g.first_row); return RL_E_INVALID; }
        if (g.n_rows < 1 || g.n_rows > g.ring_rows - g.capacity) {
            rl_set_error("%s: learner %d: n_rows must be in [1, ring_rows - capacity] = [1, %lld] (got %lld): a longer group would stamp rows of its own window",
                         who, i, g.ring_rows - g.capacity, g.n_rows);
            return RL_E_INVALID;
        }
        a.b[i] = StoreBrain{prios[i].priority, g.capacity, g.ring_rows, g.first_row, g.n_rows};
    }
    Guard guard(device_of(prios[0].priority));
    hipLaunchKernelGGL(k_prio_store_ref, dim3(n_learners), dim3(kStoreBlock), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

size_t rl_learn_prioritized_choice_work_bytes(long long capacity)
{
    if (capacity < 1 || capacity > 0x7fffffffll) return 0;
    return (size_t)(((unsigned long long)capacity * (sizeof(double) + sizeof(float)) + 255ull) / 256ull * 256ull);
}

int rl_learn_prioritized_choice(rl_world* h, const rl_learner* learners, const rl_prio* prios, const rl_prio_choice* draws, int n_learners,
                                void* stream)
{
    const char* who = "rl_learn_prioritized_choice";
    if (int rc = check_common(who, h, learners, prios, draws, n_learners)) return rc;
    ChoiceArgs a{};
    for (int i = 0; i < n_learners; ++i) {
        const rl_prio_choice& d = draws[i];
        if (int rc = check_rows(who, i, d.capacity, d.ring_rows)) return rc;
        if (d.stored < 1) { rl_set_error("%s: learner %d: stored must be >= 1 (got %lld): np.random.choice needs one row", who, i, d.stored); return RL_E_INVALID; }
        if (d.batch < 1 || d.batch > RL_LEARN_CHOICE_MAX) { rl_set_error("%s: learner %d: batch must be in [1,%d] (got %d)", who, i, RL_LEARN_CHOICE_MAX, d.batch); return RL_E_INVALID; }
        if (!d.u || !d.indices || !d.slots || !d.work) { rl_set_error("%s: learner %d: u / indices / slots / work must not be null", who, i); return RL_E_INVALID; }
        if (!(prios[i].alpha > 0.0f)) { rl_set_error("%s: prio %d: alpha must be > 0 (got %g)", who, i, (double)prios[i].alpha); return RL_E_INVALID; }
        ChoiceBrain& b = a.b[i];
        b.priority = prios[i].priority; b.u = d.u; b.indices = d.indices; b.slots = d.slots; b.bracket = d.bracket;
        b.cdf = (double*)d.work; b.w = (float*)(b.cdf + d.capacity);
        b.capacity = d.capacity; b.ring_rows = d.ring_rows; b.stored = d.stored; b.alpha = (double)prios[i].alpha; b.batch = d.batch;
    }
    a.err = h->err_flag;
    Guard guard(device_of(prios[0].priority));
    hipLaunchKernelGGL(k_prio_choice, dim3(n_learners), dim3(kChoiceBlock), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

}  // extern "C"
