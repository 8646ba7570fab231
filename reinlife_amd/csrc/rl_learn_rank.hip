// rl_learn_rank.hip -- uniform minibatch draws by content-key RANK (rl_learn_draw_rank): the rows a ring holds are sorted by their 64-bit
// content key once per call, and every draw is an index into that order.  THIS BUILD'S OWN; the reference draws with random.sample
// (ReinLife/Models/DQN.py:100).
//
// Why.  rl_learn_draw (rl_learn.hip: k_learn_pick) visits every key of a ring once per draw -- n_steps x batch x size visits of a 64-bit
// mix and compare -- and from a few hundred draws on that arithmetic, not the key pass, is its cost.  Here the cost of a call does not
// depend on n_steps x batch: one key pass, one sort, one thread per draw.
//
// The draw.  size = min(*count, capacity), read on the device.  order[0 .. size) is the rows' slots ascending by (keys[slot], slot) --
// numpy's lexsort((arange(size), keys[:size])).  Draw d = s * batch + j of learner i takes x = word 0 of rl_philox(seed, 0, i,
// (uint32)state[1], RL_SITE_LEARN, d), t = ((uint64)x * size) >> 32 and slots[d] = order[t]: rl_learn's own slots == NULL mapping, applied
// to the rank instead of the slot.  Exactly uniform up to the multiply-shift's size / 2^32, with replacement, and a function of the SET of
// rows a ring holds: equal keys are equal rows up to a 2^-64 collision, and between equal rows the lower slot comes first, which makes
// `order` a function of the ring's layout and the rows that train a function of its contents alone.  size == 0: slot 0 for every draw.
//
// The sort is a one-pass bucket sort on the keys' top 16 bits (65,536 buckets; a full ring of 50,000 rows puts 0.76 rows into a bucket on
// average) followed by an exact placement inside every bucket:
//   k_rank_clear    the histogram's 65,536 counters to zero
//   k_rank_keys     one wave per row: keys[row] = learn_row_key, and lane 0 adds 1 to hist[key >> 48]
//   k_rank_scan     one workgroup per learner: start[b] = the exclusive prefix sum of hist, and hist[b] = start[b] too (the cursors)
//   k_rank_scatter  one thread per row: tmp[atomicAdd(&hist[key >> 48], 1)] = row -- the order INSIDE a bucket's segment is the order the
//                   threads arrive in; nothing downstream depends on it.  Afterwards hist[b] is the END of bucket b's segment.
//   k_rank_place    one thread per member: its place in its bucket is the number of members with a smaller (key, slot) -- a loop over the
//                   segment, so the work is the sum of the squared bucket sizes: about 1.8 visits per row on well-mixed keys, size^2 at
//                   the worst (every row of the ring identical: one bucket, `size` iterations per thread -- bounded, and still exact).
//   k_rank_pick     one thread per draw
// Six launches whatever n_steps, the batches and the rings hold.  The only atomics are integer adds, and every value the caller sees
// (keys, order, slots) is independent of the order they arrive in: the same bits in every run.
//
// The prioritised memories' draws by the same order (rl_learn_prioritized_draw_rank, rl_learn_td_draw_rank: a cumulative sum of the
// weights in rank order, one binary search per draw) follow the uniform draw below and reuse its sort kernels as they are.
#include "rl_learn_dev.h"

namespace {

constexpr int kRankSite = RL_SITE_LEARN;
constexpr int kRankBits = 16;                          // the keys' top bits that name a bucket
constexpr int kRankBuckets = 1 << kRankBits;
constexpr int kRankShift = 64 - kRankBits;
constexpr int kScanBlock = 1024;
constexpr int kScanPer = kRankBuckets / kScanBlock;    // counters per thread of the scan: 64, read as 16 uint4
constexpr size_t kRankTableBytes = (size_t)kRankBuckets * sizeof(uint32_t);

// a learner's work buffer: hist[65536] | start[65536] | tmp[capacity] (uint32 / uint32 / int32), 16-byte aligned
struct RankBrain {
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const int32_t* r_age;
    const unsigned long long* r_count;
    long long r_capacity;
    unsigned long long* keys;    // [capacity]
    int32_t* order;              // [capacity]
    uint32_t *hist, *start;      // [65536] each
    int32_t* tmp;                // [capacity]
    const long long* state;      // rl_learner.state ([1] = calls made)
    long long slots0;            // where this learner's [n_steps][batch] table starts in `slots`
    int batch;
};
struct RankArgs {
    RankBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* slots;              // the learners' [n_steps][batch] tables, end to end
    uint64_t seed;
    int n_steps;
};

__device__ inline long long rank_size(const RankBrain& B)
{
    const unsigned long long count = *B.r_count;
    return count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
}

// 64 workgroups per learner: 16,384 uint4 of zeros
__global__ __launch_bounds__(256) void k_rank_clear(const RankArgs A)
{
    uint4* h = (uint4*)A.b[blockIdx.y].hist;
    h[blockIdx.x * 256 + threadIdx.x] = uint4{0u, 0u, 0u, 0u};
}

// one wave per ring row: keys[row], and the row counted in its bucket
__global__ __launch_bounds__(256) void k_rank_keys(const RankArgs A)
{
    const RankBrain& B = A.b[blockIdx.y];
    const long long size = rank_size(B);
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= size) return;
    const uint64_t k = learn_row_key(B.r_state, B.r_state_prime, B.r_action, B.r_reward, B.r_done, B.r_age, row, lane);
    if (lane == 0) {
        B.keys[row] = k;
        atomicAdd(&B.hist[k >> kRankShift], 1u);
    }
}

// one workgroup per learner: the exclusive prefix sum of the 65,536 counters into start[] and back into hist[] (the scatter's cursors)
__global__ __launch_bounds__(kScanBlock) void k_rank_scan(const RankArgs A)
{
    __shared__ uint32_t part[kScanBlock];
    const RankBrain& B = A.b[blockIdx.x];
    const int tid = threadIdx.x;
    uint4* h4 = (uint4*)(B.hist + (size_t)tid * kScanPer);
    uint4* s4 = (uint4*)(B.start + (size_t)tid * kScanPer);
    uint32_t sum = 0;
#pragma unroll 4
    for (int i = 0; i < kScanPer / 4; ++i) { const uint4 v = h4[i]; sum += v.x + v.y + v.z + v.w; }
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < kScanBlock; o <<= 1) {   // inclusive scan of the threads' sums
        const uint32_t v = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
#pragma unroll 4
    for (int i = 0; i < kScanPer / 4; ++i) {
        const uint4 v = h4[i];
        uint4 e;
        e.x = run; run += v.x;
        e.y = run; run += v.y;
        e.z = run; run += v.z;
        e.w = run; run += v.w;
        s4[i] = e; h4[i] = e;
    }
}

// one thread per ring row: the row's slot into its bucket's segment of tmp, at the place the cursor hands out
__global__ __launch_bounds__(256) void k_rank_scatter(const RankArgs A)
{
    const RankBrain& B = A.b[blockIdx.y];
    const long long size = rank_size(B);
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= size) return;
    const uint32_t p = atomicAdd(&B.hist[B.keys[row] >> kRankShift], 1u);
    if ((long long)p < size) B.tmp[p] = (int32_t)row;   // (always, while the ring's counter stands still between the launches of a call)
}

// one thread per member of tmp: order[bucket start + the number of the bucket's members with a smaller (key, slot)] = slot
__global__ __launch_bounds__(256) void k_rank_place(const RankArgs A)
{
    const RankBrain& B = A.b[blockIdx.y];
    const long long size = rank_size(B);
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= size) return;
    const int32_t slot = B.tmp[p];
    if (slot < 0 || slot >= size) return;               // (never, see k_rank_scatter: no address is formed from a value out of range)
    const uint64_t key = B.keys[slot];
    const uint32_t b = (uint32_t)(key >> kRankShift);
    const long long lo = B.start[b];
    long long hi = B.hist[b];                           // the cursor after the scatter: the end of the segment
    if (hi > size) hi = size;
    long long below = 0;
    for (long long q = lo; q < hi; ++q) {
        const int32_t other = B.tmp[q];
        if (other < 0 || other >= size) continue;
        const uint64_t ko = B.keys[other];
        below += (ko < key || (ko == key && other < slot)) ? 1 : 0;
    }
    if (lo + below < size) B.order[lo + below] = slot;
}

// one thread per draw: slots[d] = order[rank the draw's Philox word names]
__global__ __launch_bounds__(256) void k_rank_pick(const RankArgs A)
{
    const int brain = blockIdx.y;
    const RankBrain& B = A.b[brain];
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d >= (long long)A.n_steps * B.batch) return;
    const long long size = rank_size(B);
    int32_t slot = 0;
    if (size > 0) {
        const uint32_t x = rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)B.state[1], (uint32_t)kRankSite, (uint32_t)d).x;
        slot = B.order[((uint64_t)x * (uint64_t)size) >> 32];
    }
    A.slots[B.slots0 + d] = slot;
}

// ---- prioritised draws by prefix sum over content-key rank (rl_learn_prioritized_draw_rank, rl_learn_td_draw_rank) -------------------
// THIS BUILD'S OWN sampler beside rl_learn_prio.hip's exponential race (one workgroup per draw, each a pass over the ring).  With `order`
// fixed, a prioritised draw is a cumulative sum of the weights in rank order and one binary search per draw: the cost of a call does not
// depend on n_steps x batch, the probabilities are w_i / sum w exactly (up to the sum's rounding), and with one uniform per segment of
// total / batch it is the reference's stratified Memory.sample() (PERDQN.py:280-304).  The sort is the uniform draw's, kernel for kernel:
//   k_rank_clear      as above
//   k_prank_keys      k_rank_keys and rl_learn_prio.hip's k_prio_prepare in one pass: the stamp, weight = priority^alpha (TD: none), key, bucket
//   k_rank_scan / k_rank_scatter / k_rank_place   as above: order[0 .. size)
//   k_prank_segments  one wave per segment of kPrankSeg = 64 consecutive ranks: w_r = (double)weight[order[r]] where that is > 0, else 0
//                     (a NaN too); local[r] = the inclusive left-to-right sum of the segment's w up to r, into cum[r]; the segment's total
//   k_prank_base      one workgroup per learner: base[s] = the exclusive left-to-right sum of the totals (one thread adds them), then
//                     cum[r] = base[r / 64] + local[r] -- a fixed association order: the same bits in every run
//   k_prank_pick      one thread per draw d = s * batch + j: r4 = rl_philox(seed, 0, i, (uint32)state[1], site, d); u = (double)((r4.y : r4.x)
//                     >> 11) * 2^-53; target = u * total, stratified ((double)j + u) * (total / batch), each one rounded operation after the
//                     other; the smallest rank r with cum[r] > target (none: the smallest with cum[r] == total); total == 0 or not finite:
//                     the uniform rank draw order[(r4.x * size) >> 32]; size == 0: slot 0.  Draw 0 advances *seen to *count.
// Eight launches whatever n_steps, the batches and the rings hold; integer atomics only.
constexpr int kPrankSeg = 64;

struct PrankBrain {
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const int32_t* r_age;
    const unsigned long long* r_count;
    long long r_capacity;
    float *priority, *weight;    // (TD: weight is null)
    const float* wsrc;           // what a draw is proportional to: weight (TD: priority)
    const float* prio_max;       // (TD: null)
    unsigned long long* seen;
    unsigned long long* keys;    // [capacity]
    const int32_t* order;        // [capacity], written by k_rank_place
    uint32_t* hist;              // [65536]: the buckets' counters
    double* cum;                 // [capacity]
    double* seg;                 // [ceil(capacity / 64)]: the segments' totals, then their bases
    const long long* state;      // rl_learner.state ([1] = calls made)
    long long slots0;            // where this learner's [n_steps][batch] table starts in `slots`
    float p_new;                 // (TD only)
    float alpha;
    int batch;
};
struct PrankArgs {
    PrankBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* slots;              // the learners' [n_steps][batch] tables, end to end
    uint64_t seed;
    int n_steps;
    int stratified;
    int site;                    // RL_SITE_LEARN_PRIO or RL_SITE_LEARN_TD: the race draws' own sites
};
static_assert(sizeof(RankArgs) <= 4096, "kernel arguments are passed by value");
static_assert(sizeof(PrankArgs) <= 4096, "kernel arguments are passed by value");

__device__ inline long long prank_size(const PrankBrain& B)
{
    const unsigned long long count = *B.r_count;
    return count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
}

// one wave per ring row: k_prio_prepare's stamp and weight (rl_learn_prio.hip, unchanged), keys[row], and the row counted in its bucket
template <bool TD>
__global__ __launch_bounds__(256) void k_prank_keys(const PrankArgs A)
{
    const PrankBrain& B = A.b[blockIdx.y];
    const unsigned long long count = *B.r_count, seen = *B.seen, cap = (unsigned long long)B.r_capacity;
    const long long size = count < cap ? (long long)count : B.r_capacity;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= size) return;
    const uint64_t k = learn_row_key(B.r_state, B.r_state_prime, B.r_action, B.r_reward, B.r_done, B.r_age, row, lane);
    if (lane == 0) {
        const unsigned long long fresh = count > seen ? count - seen : 0ull;          // rows appended since the last draw
        const unsigned long long behind = ((unsigned long long)row + cap - seen % cap) % cap;   // slots from seen's to this row's, going round
        const bool stamp = fresh >= cap || behind < fresh;
        if (TD) {
            if (stamp) B.priority[row] = B.p_new;
        } else {
            float p;
            if (stamp) { p = *B.prio_max; B.priority[row] = p; }
            else p = B.priority[row];
            B.weight[row] = B.alpha == 1.0f ? p : powf(p, B.alpha);   // (rl_learn_prio.hip's k_prio_prepare: powf(p, 1.0f) is up to 1 ulp off p)
        }
        B.keys[row] = k;
        atomicAdd(&B.hist[k >> kRankShift], 1u);
    }
}

// one wave per segment of 64 consecutive ranks, one lane per rank: the loads side by side, the sum left to right
__global__ __launch_bounds__(256) void k_prank_segments(const PrankArgs A)
{
    const PrankBrain& B = A.b[blockIdx.y];
    const long long size = prank_size(B);
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s * kPrankSeg >= size) return;                    // (the whole wave)
    const long long r = s * kPrankSeg + lane;
    double w = 0.0;
    if (r < size) {
        const int32_t slot = B.order[r];
        if (slot >= 0 && slot < size) {                   // (always: order[0 .. size) is a permutation of the slots)
            const float f = B.wsrc[slot];
            if (f > 0.0f) w = (double)f;                  // a zero, negative or NaN weight counts as 0
        }
    }
    const int lo = __double2loint(w), hi = __double2hiint(w);
    double run = 0.0, mine = 0.0;
#pragma unroll
    for (int i = 0; i < kPrankSeg; ++i) {
        run = __dadd_rn(run, __hiloint2double(__builtin_amdgcn_readlane(hi, i), __builtin_amdgcn_readlane(lo, i)));
        if (lane == i) mine = run;
    }
    if (r < size) B.cum[r] = mine;
    if (lane == 0) B.seg[s] = run;                        // (the ranks past `size` added zeros)
}

// one workgroup per learner: the segments' totals to their exclusive sums, added by ONE thread in segment order; then cum = base + local
__global__ __launch_bounds__(256) void k_prank_base(const PrankArgs A)
{
    __shared__ double part[256];
    const PrankBrain& B = A.b[blockIdx.x];
    const long long size = prank_size(B);
    const long long n_seg = (size + kPrankSeg - 1) / kPrankSeg;
    const int tid = threadIdx.x;
    double run = 0.0;                                     // (thread 0's)
    for (long long c = 0; c < n_seg; c += 256) {
        if (c + tid < n_seg) part[tid] = B.seg[c + tid];
        __syncthreads();
        if (tid == 0) {
            const int n = n_seg - c < 256 ? (int)(n_seg - c) : 256;
            for (int k = 0; k < n; ++k) { const double t = part[k]; part[k] = run; run = __dadd_rn(run, t); }
        }
        __syncthreads();
        if (c + tid < n_seg) B.seg[c + tid] = part[tid];
        __syncthreads();
    }
    for (long long r = tid; r < size; r += 256) B.cum[r] = __dadd_rn(B.seg[r / kPrankSeg], B.cum[r]);
}

// one thread per draw: a binary search in cum
__global__ __launch_bounds__(256) void k_prank_pick(const PrankArgs A)
{
    const int brain = blockIdx.y;
    const PrankBrain& B = A.b[brain];
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d >= (long long)A.n_steps * B.batch) return;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    if (d == 0) *B.seen = count;                          // (k_prank_keys, the only reader, is a launch in front of this one)
    int32_t slot = 0;
    if (size > 0) {
        const rl_u4 r4 = rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)B.state[1], (uint32_t)A.site, (uint32_t)d);
        const double total = B.cum[size - 1];
        long long rank;
        if (!(total > 0.0) || !(total <= 1.7976931348623157e308)) {               // every weight zero, or a sum that is not finite: uniform
            rank = (long long)(((uint64_t)r4.x * (uint64_t)size) >> 32);
        } else {
            const uint64_t x = (((uint64_t)r4.y << 32) | r4.x) >> 11;
            const double u = __dmul_rn((double)x, 1.1102230246251565e-16);         // x * 2^-53: exact, in [0, 1)
            double target;
            if (A.stratified) {
                const double seg = __ddiv_rn(total, (double)B.batch);
                target = __dmul_rn(__dadd_rn((double)(d % B.batch), u), seg);
            } else {
                target = __dmul_rn(u, total);
            }
            long long lo = 0, hi = size;                  // the smallest rank with cum > target
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (B.cum[mid] > target) hi = mid; else lo = mid + 1;
            }
            if (lo >= size) {                             // rounding gave target >= total: the smallest rank with cum == total
                lo = 0; hi = size - 1;
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (B.cum[mid] >= total) hi = mid; else lo = mid + 1;
                }
            }
            rank = lo;
        }
        slot = B.order[rank];
    }
    A.slots[B.slots0 + d] = slot;
}

}  // namespace

size_t rl_learn_draw_rank_work_bytes_impl(long long capacity)
{
    return 2 * kRankTableBytes + (((size_t)capacity * sizeof(int32_t) + 15) & ~(size_t)15);
}

int rl_learn_draw_rank_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps,
                              unsigned long long* const* keys, int32_t* const* order, void* const* work, int32_t* slots, hipStream_t stream)
{
    RankArgs a{};
    long long max_cap = 1, slots0 = 0;
    int max_batch = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        RankBrain& b = a.b[i];
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done; b.r_age = r.age;
        b.r_count = r.count; b.r_capacity = r.capacity; b.keys = keys[i]; b.order = order[i];
        b.hist = (uint32_t*)work[i]; b.start = b.hist + kRankBuckets; b.tmp = (int32_t*)(b.start + kRankBuckets);
        b.state = (const long long*)learners[i].state; b.batch = learners[i].batch; b.slots0 = slots0;
        slots0 += (long long)n_steps * b.batch;
        max_cap = r.capacity > max_cap ? r.capacity : max_cap;
        max_batch = b.batch > max_batch ? b.batch : max_batch;
    }
    a.slots = slots; a.seed = h->cfg.seed; a.n_steps = n_steps;
    const unsigned row_blocks = (unsigned)((max_cap + 255) / 256);
    const unsigned draw_blocks = (unsigned)(((long long)n_steps * max_batch + 255) / 256);
    hipLaunchKernelGGL(k_rank_clear, dim3(kRankBuckets / 4 / 256, n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)((max_cap + 3) / 4), n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_rank_scan, dim3(n_learners), dim3(kScanBlock), 0, stream, a);
    hipLaunchKernelGGL(k_rank_scatter, dim3(row_blocks, n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_rank_place, dim3(row_blocks, n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_rank_pick, dim3(draw_blocks, n_learners), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("rl_learn_draw_rank: kernel launch failed: %s", hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

size_t rl_learn_prio_draw_rank_work_bytes_impl(long long capacity)
{
    const size_t n_seg = ((size_t)capacity + kPrankSeg - 1) / kPrankSeg;
    return rl_learn_draw_rank_work_bytes_impl(capacity) + ((n_seg * sizeof(double) + 15) & ~(size_t)15);
}

// prios (PERD3QN) or tds (PERDQN), the other null: hist | start | tmp | the segments' sums in work[i]
static int prank_launch(const char* who, rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, const rl_tdprio* tds,
                        int n_learners, int n_steps, int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots,
                        hipStream_t stream)
{
    RankArgs s{};       // the sort's view of the same buffers
    PrankArgs a{};
    long long max_cap = 1, slots0 = 0;
    int max_batch = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        RankBrain& sb = s.b[i];
        PrankBrain& b = a.b[i];
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done; b.r_age = r.age;
        b.r_count = r.count; b.r_capacity = r.capacity;
        if (tds) { b.priority = tds[i].priority; b.wsrc = tds[i].priority; b.keys = tds[i].keys; b.seen = tds[i].seen; b.p_new = tds[i].p_new; }
        else { const rl_prio& p = prios[i]; b.priority = p.priority; b.weight = p.weight; b.wsrc = p.weight; b.keys = p.keys; b.prio_max = p.prio_max; b.seen = p.seen; b.alpha = p.alpha; }
        sb.r_count = r.count; sb.r_capacity = r.capacity; sb.keys = b.keys; sb.order = order[i];
        sb.hist = (uint32_t*)work[i]; sb.start = sb.hist + kRankBuckets; sb.tmp = (int32_t*)(sb.start + kRankBuckets);
        b.order = order[i]; b.hist = sb.hist; b.cum = cum[i];
        b.seg = (double*)((char*)work[i] + rl_learn_draw_rank_work_bytes_impl(r.capacity));
        b.state = (const long long*)learners[i].state; b.batch = learners[i].batch; b.slots0 = slots0;
        slots0 += (long long)n_steps * b.batch;
        max_cap = r.capacity > max_cap ? r.capacity : max_cap;
        max_batch = b.batch > max_batch ? b.batch : max_batch;
    }
    a.slots = slots; a.seed = h->cfg.seed; a.n_steps = n_steps; a.stratified = stratified ? 1 : 0;
    a.site = tds ? RL_SITE_LEARN_TD : RL_SITE_LEARN_PRIO;
    const unsigned row_blocks = (unsigned)((max_cap + 255) / 256);
    const unsigned seg_blocks = (unsigned)(((max_cap + kPrankSeg - 1) / kPrankSeg + 3) / 4);
    const unsigned draw_blocks = (unsigned)(((long long)n_steps * max_batch + 255) / 256);
    hipLaunchKernelGGL(k_rank_clear, dim3(kRankBuckets / 4 / 256, n_learners), dim3(256), 0, stream, s);
    if (tds) hipLaunchKernelGGL(k_prank_keys<true>, dim3((unsigned)((max_cap + 3) / 4), n_learners), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_prank_keys<false>, dim3((unsigned)((max_cap + 3) / 4), n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_rank_scan, dim3(n_learners), dim3(kScanBlock), 0, stream, s);
    hipLaunchKernelGGL(k_rank_scatter, dim3(row_blocks, n_learners), dim3(256), 0, stream, s);
    hipLaunchKernelGGL(k_rank_place, dim3(row_blocks, n_learners), dim3(256), 0, stream, s);
    hipLaunchKernelGGL(k_prank_segments, dim3(seg_blocks, n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_prank_base, dim3(n_learners), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_prank_pick, dim3(draw_blocks, n_learners), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: kernel launch failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

int rl_learn_prioritized_draw_rank_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                                          int n_steps, int stratified, int32_t* const* order, double* const* cum, void* const* work,
                                          int32_t* slots, hipStream_t stream)
{
    return prank_launch("rl_learn_prioritized_draw_rank", h, learners, rings, prios, nullptr, n_learners, n_steps, stratified, order, cum, work, slots, stream);
}

int rl_learn_td_draw_rank_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners,
                                 int n_steps, int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots,
                                 hipStream_t stream)
{
    return prank_launch("rl_learn_td_draw_rank", h, learners, rings, nullptr, tds, n_learners, n_steps, stratified, order, cum, work, slots, stream);
}

// rl_learn_td_wide_draw_rank: the same eight launches for batches up to RL_LEARN_TD_WIDE_MAX (one thread per draw d = s * batch + j, salted
// by d; stratified cuts the total into `batch` segments) -- at batch <= 64 rl_learn_td_draw_rank's table, bit for bit.
int rl_learn_td_wide_draw_rank_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners,
                                      int n_steps, int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots,
                                      hipStream_t stream)
{
    return prank_launch("rl_learn_td_wide_draw_rank", h, learners, rings, nullptr, tds, n_learners, n_steps, stratified, order, cum, work, slots, stream);
}
