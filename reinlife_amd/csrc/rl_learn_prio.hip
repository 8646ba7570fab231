// rl_learn_prio.hip -- the prioritised memory's draw on the device (rl_learn_prioritized_draw): the minibatches of a PERD3QN brain, drawn
// with probability priority^alpha / sum from the replay rings rl_run_ex / rl_capture_transitions fill, with no host round trip.
//
// Reference (ReinLife/Models/PERD3QN.py):
//   PrioritizedReplayBuffer.store    :143-155  a new row gets max(priorities), 1.0 into an empty memory
//   PrioritizedReplayBuffer.sample   :157-165  np.random.choice(len, batch, p = priorities^alpha / sum): WITH replacement
//   update_priorities                :177-179  (made by k_learn_d3qn<true>, rl_learn_dueling.hip)
//
// Stamping.  The rings know nothing of priorities, and need not: store() never lowers the maximum (a row overwritten with the maximum
// keeps it), so between two learning calls the maximum is a constant, and a ring's slots are count mod capacity.  "Every row appended
// since the last draw gets the current maximum" is therefore done here, after the fact: k_prio_prepare stamps the slots of
// [*seen, *count) mod capacity (all rows once count - seen >= capacity) with *prio_max, and k_prio_pick -- a later launch, which does
// not read `seen` -- advances *seen to *count.
//
// Draw.  Like rl_learn_draw's, it must not name a slot: the multi-tick launch appends the worlds' rows in the order their workgroups
// reach an atomic counter.  Every row has its 64-bit content key (learn_row_key); draw d mixes it with the draw's own 64 Philox bits to
// v, makes a uniform U in (0,1) of v's top 23 bits and t = -logf(U) / weight, an exponential variate of rate weight, and takes the row
// with the smallest (t, v, slot).  The minimum of independent exponentials falls on row i with probability w_i / sum w: sampling with
// replacement, the same rows whatever slots they sit in -- as far as mix64 behaves like a random function (tests/test_hip_learn_perd3qn.py
// counts 6,400 draws over 48 rows).  U has 23 bits, so on a ring of N rows the winning t is about 2^23 / N grid steps from zero: the
// probabilities are the exact race's up to about N / 2^23 of themselves, and equal t are told apart by v.  A weight that is zero (or NaN)
// gives t = +inf -- and so does a positive weight below about 4.9e-38, where -logf(U) / weight (at most 16.7 / weight) overflows: such a row
// ranks with the zero-weight rows, by v.  With alpha = 0.6 no float priority is that small (the smallest denormal has weight 1.2e-27); an
// alpha above about 0.84 can reach it with denormal priorities.  If every weight is zero the order is v's alone: rl_learn_draw's uniform
// draw (the reference would raise).
#include "rl_learn_dev.h"

#include <math.h>

namespace {

// The same two kernels serve the PERDQN memory (rl_learn_td_draw, TD = true; PERDQN.py's Memory / SumTree): its new rows are stamped with
// a constant (rl_tdprio.p_new: append_sample's priority is (0 + e) ** a whatever the row, rl_learn_td.hip), and the race weight is the
// stored priority itself, which already carries ** a -- no powf, no weight column.  Salts from RL_SITE_LEARN_TD.

struct PrioBrain {
    const float *r_state, *r_state_prime, *r_reward;
    const int8_t* r_action;
    const uint8_t* r_done;
    const int32_t* r_age;
    const unsigned long long* r_count;
    long long r_capacity;
    float *priority, *weight;
    unsigned long long* keys;
    const float* prio_max;       // (TD: null)
    float p_new;                 // (TD only)
    unsigned long long* seen;
    const long long* state;      // rl_learner.state ([1] = calls made)
    float alpha;
    int batch;
};
struct PrioArgs {
    PrioBrain b[RL_MAX_CAPTURE_BRAINS];
    int32_t* slots;              // the learners' [n_steps][batch] tables, end to end
    uint64_t seed;
    int n_steps;
};

// one wave per ring row: the stamp, weight[row] = priority[row]^alpha (TD: none), keys[row]
// (rl_learn_rank.hip's k_prank_keys repeats this body and adds the bucket count: a change of the stamp or weight rule goes to both;
// tests/test_hip_learn_prio_draw_rank.py compares what the two leave, bit for bit)
template <bool TD>
__global__ __launch_bounds__(256) void k_prio_prepare(const PrioArgs A)
{
    const PrioBrain& B = A.b[blockIdx.y];
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
            B.weight[row] = B.alpha == 1.0f ? p : powf(p, B.alpha);   // (the device powf(p, 1.0f) is up to 1 ulp off p)
        }
        B.keys[row] = k;
    }
}

__device__ inline bool prio_less(float t, uint64_t v, int i, float bt, uint64_t bv, int bi)
{
    return t < bt || (t == bt && (v < bv || (v == bv && i < bi)));
}

// one workgroup per draw: slots[brain][d] = the row with the smallest (t, v, slot)
template <bool TD>
__global__ __launch_bounds__(256) void k_prio_pick(const PrioArgs A)
{
    __shared__ float best_t[256];
    __shared__ uint64_t best_v[256];
    __shared__ int best_i[256];
    const int brain = blockIdx.y, d = blockIdx.x, tid = threadIdx.x;
    const PrioBrain& B = A.b[brain];
    if (d >= A.n_steps * B.batch) return;
    const unsigned long long count = *B.r_count;
    const long long size = count < (unsigned long long)B.r_capacity ? (long long)count : B.r_capacity;
    if (d == 0 && tid == 0) *B.seen = count;   // (k_prio_prepare, the only reader, is the launch in front of this one)
    const rl_u4 r = rl_philox4x32(A.seed, 0u, (uint32_t)brain, (uint32_t)B.state[1], (uint32_t)(TD ? RL_SITE_LEARN_TD : RL_SITE_LEARN_PRIO), (uint32_t)d);
    const uint64_t salt = ((uint64_t)r.y << 32) | r.x;
    float bt = INFINITY;
    uint64_t bv = ~0ull;
    int bi = 0x7fffffff;
    for (long long i = tid; i < size; i += 256) {
        const uint64_t v = learn_mix64(B.keys[i] ^ salt);
        const float w = TD ? B.priority[i] : B.weight[i];
        const float u = ((float)(uint32_t)(v >> 41) + 0.5f) * (1.0f / 8388608.0f);   // exact: 24 significant bits, in [2^-24, 1 - 2^-24]
        const float t = w > 0.0f ? -logf(u) / w : INFINITY;                         // (a NaN weight: +inf too)
        if (prio_less(t, v, (int)i, bt, bv, bi)) { bt = t; bv = v; bi = (int)i; }
    }
    best_t[tid] = bt; best_v[tid] = bv; best_i[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o && prio_less(best_t[tid + o], best_v[tid + o], best_i[tid + o], best_t[tid], best_v[tid], best_i[tid])) {
            best_t[tid] = best_t[tid + o]; best_v[tid] = best_v[tid + o]; best_i[tid] = best_i[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int batch0 = 0;   // (the learners' rows of `slots` are [n_steps][batch] each, laid end to end)
        for (int b = 0; b < brain; ++b) batch0 += A.n_steps * A.b[b].batch;
        A.slots[batch0 + d] = (size > 0 && best_i[0] < size) ? best_i[0] : 0;
    }
}

}  // namespace

template <bool TD>
static int prio_draw_launch(const char* who, rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, const rl_tdprio* tds,
                            int n_learners, int n_steps, int32_t* slots, hipStream_t stream)
{
    PrioArgs a{};
    long long max_cap = 1;
    int max_batch = 1;
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        PrioBrain& b = a.b[i];
        b.r_state = r.state; b.r_state_prime = r.state_prime; b.r_reward = r.reward; b.r_action = r.action; b.r_done = r.done; b.r_age = r.age;
        b.r_count = r.count; b.r_capacity = r.capacity;
        if (TD) { b.priority = tds[i].priority; b.keys = tds[i].keys; b.seen = tds[i].seen; b.p_new = tds[i].p_new; }
        else { const rl_prio& p = prios[i]; b.priority = p.priority; b.weight = p.weight; b.keys = p.keys; b.prio_max = p.prio_max; b.seen = p.seen; b.alpha = p.alpha; }
        b.state = (const long long*)learners[i].state; b.batch = learners[i].batch;
        max_cap = r.capacity > max_cap ? r.capacity : max_cap;
        max_batch = b.batch > max_batch ? b.batch : max_batch;
    }
    a.slots = slots; a.seed = h->cfg.seed; a.n_steps = n_steps;
    hipLaunchKernelGGL(k_prio_prepare<TD>, dim3((unsigned)((max_cap + 3) / 4), n_learners), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: launch of the prepare kernel failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    hipLaunchKernelGGL(k_prio_pick<TD>, dim3(n_steps * max_batch, n_learners), dim3(256), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("%s: launch of the pick kernel failed: %s", who, hipGetErrorString(e)); return RL_E_LAUNCH; }
    return RL_OK;
}

int rl_learn_prioritized_draw_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                                     int n_steps, int32_t* slots, hipStream_t stream)
{
    return prio_draw_launch<false>("rl_learn_prioritized_draw", h, learners, rings, prios, nullptr, n_learners, n_steps, slots, stream);
}

// rl_learn_prioritized_wide_draw: the same two launches for batches up to RL_LEARN_PRIORITIZED_WIDE_MAX (the kernels are written over any
// batch: one workgroup per draw d = s * batch + j, salted by d) -- at batch <= 64 rl_learn_prioritized_draw's table, bit for bit.
int rl_learn_prioritized_wide_draw_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                                          int n_steps, int32_t* slots, hipStream_t stream)
{
    return prio_draw_launch<false>("rl_learn_prioritized_wide_draw", h, learners, rings, prios, nullptr, n_learners, n_steps, slots, stream);
}

int rl_learn_td_draw_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners,
                            int n_steps, int32_t* slots, hipStream_t stream)
{
    return prio_draw_launch<true>("rl_learn_td_draw", h, learners, rings, nullptr, tds, n_learners, n_steps, slots, stream);
}

// rl_learn_td_wide_draw: the same two launches for batches up to RL_LEARN_TD_WIDE_MAX (one workgroup per draw d = s * batch + j, salted
// by d) -- at batch <= 64 rl_learn_td_draw's table, bit for bit.
int rl_learn_td_wide_draw_launch(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners,
                                 int n_steps, int32_t* slots, hipStream_t stream)
{
    return prio_draw_launch<true>("rl_learn_td_wide_draw", h, learners, rings, nullptr, tds, n_learners, n_steps, slots, stream);
}
