// rl_learn_dev.h -- what the learning units (rl_learn.hip: k_learn_dqn, rl_learn_dueling.hip: k_learn_d3qn, rl_learn_prio.hip: the prioritised draws,
// rl_learn_td.hip: k_learn_perdqn) share: torch's Adam update of one parameter, the toward-zero f16 split of rl_policy.hip's host packer on the
// device and its to-nearest counterpart (PERDQN), the packed layouts' index rule, the
// content key of a ring row and the decimal a float hyperparameter stands for.  Everything is inline in an unnamed namespace: each unit gets its own copy.
#pragma once
#include "rl_policy_dev.h"

#include <stdio.h>
#include <stdlib.h>

namespace {

struct AdamStep {
    float *p, *m, *v, *grad;   // grad: this step's row of the caller's buffer or null
    double w1, w2, beta2, bc2_sqrt, eps, neg_step;
};
// torch.optim.Adam's single-tensor update: exp_avg.lerp_(g, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g, value = 1 - b2);
// denom = exp_avg_sq.sqrt() / sqrt(1 - b2^t) + eps; param.addcdiv_(exp_avg, denom, value = -lr / (1 - b1^t))
// The arithmetic of one parameter is double and each of p, m, v is rounded to float ONCE: moments of a run that is under way make
// m / sqrt(v) reach thousands (a step of thousands of lr) and let m + w1 (g - m) cancel, where float roundings of the intermediate values
// are no longer small against 1e-5 lr or an ulp of the result (tests/test_hip_learn_edges.py, Adam at step 10,000).  The decimal
// hyperparameters stay double throughout.
__device__ inline void adam_update(const AdamStep& a, int idx, float g)
{
    if (a.grad) a.grad[idx] = g;
    const double gd = (double)g;
    double m = (double)a.m[idx], v = (double)a.v[idx];
    m = m + a.w1 * (gd - m);
    v = v * a.beta2 + (a.w2 * gd) * gd;
    const double denom = sqrt(v) / a.bc2_sqrt + a.eps;
    a.m[idx] = (float)m; a.v[idx] = (float)v;
    a.p[idx] = (float)((double)a.p[idx] + (a.neg_step * m) / denom);
}

// ---- the toward-zero f16 split of rl_policy.hip's host packer (f16_rtz, f16_to_float, split2_host), on the device ----
__device__ inline uint32_t learn_f16_rtz(float f)
{
    const uint32_t u = __float_as_uint(f);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int e = (int)((u >> 23) & 0xff) - 127;
    const uint32_t man = u & 0x7fffffu;
    if (e < -24) return sign;
    if (e < -14) return sign | ((man | 0x800000u) >> (13 + (-14 - e)));
    return sign | (uint32_t)((e + 15) << 10) | (man >> 13);
}
__device__ inline float learn_f16_to_float(uint32_t h)
{
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1f, man = h & 0x3ffu;
    if (e == 0) return __uint_as_float(__float_as_uint((float)man * (1.0f / 16777216.0f)) | sign);
    return __uint_as_float(sign | ((e - 15 + 127) << 23) | (man << 13));
}
// one fragment of 8 scaled weights -> its hi and lo planes (16 bytes each)
__device__ inline void learn_store_fragment(const float (&x)[8], uint4* hi_dst, uint4* lo_dst)
{
    uint32_t hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = learn_f16_rtz(x[e]);
        lo[e] = learn_f16_rtz(x[e] - learn_f16_to_float(hi[e]));   // (the subtraction is exact)
    }
    *hi_dst = uint4{hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16)};
    *lo_dst = uint4{lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16)};
}
// ---- ... and the split to the NEAREST f16, ties to even (f16_rne, split2_host with rne: PERDQN's packed weights alone) ----
__device__ inline uint32_t learn_f16_rne(float f)
{
    const uint32_t u = __float_as_uint(f);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int e = (int)((u >> 23) & 0xff) - 127;
    if (e < -25) return sign;                                         // below half the smallest subnormal
    const int eq = e < -14 ? -14 : e;                                 // exponent of the f16 quantum 2^(eq - 10)
    const int shift = 13 + (eq - e);
    const uint32_t man = (u & 0x7fffffu) | 0x800000u;
    uint32_t r = man >> shift;
    const uint32_t rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) ++r;                 // (a carry into the exponent is the right result)
    return sign | (uint32_t)(((eq + 14) << 10) + r);
}
__device__ inline void learn_store_fragment_rne(const float (&x)[8], uint4* hi_dst, uint4* lo_dst)
{
    uint32_t hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = learn_f16_rne(x[e]);
        lo[e] = learn_f16_rne(x[e] - learn_f16_to_float(hi[e]));   // (the subtraction is exact)
    }
    *hi_dst = uint4{hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16)};
    *lo_dst = uint4{lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16)};
}
__device__ inline int learn_hidden_k(int t, int c, int e, int lane) { const int r = 8 * c + e; return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ---- the content key of a ring row (rl_learn_draw, rl_learn_prioritized_draw): a sum of mixed (position, bits) terms, so any summation
// order gives the same key ----
__device__ inline uint64_t learn_mix64(uint64_t z)   // splitmix64's finalizer
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline uint64_t learn_term(int position, uint32_t bits) { return learn_mix64(((uint64_t)(position + 1) << 32) | bits); }
// by one whole wave (lane 0..63): the terms of state (positions 0..152), state_prime (153..305), action, reward, done, age; every lane
// returns the key
__device__ inline uint64_t learn_row_key(const float* r_state, const float* r_state_prime, const int8_t* r_action, const float* r_reward,
                                         const uint8_t* r_done, const int32_t* r_age, long long row, int lane)
{
    uint64_t k = 0;
    for (int f = lane; f < RL_OBS_DIM; f += 64) {
        k += learn_term(f, __float_as_uint(r_state[(size_t)row * RL_OBS_DIM + f]));
        k += learn_term(RL_OBS_DIM + f, __float_as_uint(r_state_prime[(size_t)row * RL_OBS_DIM + f]));
    }
    if (lane == 0) k += learn_term(2 * RL_OBS_DIM, (uint32_t)(uint8_t)r_action[row]) + learn_term(2 * RL_OBS_DIM + 1, __float_as_uint(r_reward[row]))
                      + learn_term(2 * RL_OBS_DIM + 2, (uint32_t)r_done[row]) + learn_term(2 * RL_OBS_DIM + 3, (uint32_t)r_age[row]);
    for (int o = 32; o > 0; o >>= 1) k += __shfl_xor((unsigned long long)k, o);
    return k;
}

// The decimal a float hyperparameter stands for (0.999f -> 0.999, not 0.99900001287): torch computes Adam's bias corrections from the
// Python doubles, and 1 - 0.999f^t differs from 1 - 0.999^t by 1.3e-5 of itself at t = 1.
inline double learn_decimal(float f)
{
    char buf[40];
    snprintf(buf, sizeof(buf), "%.7g", (double)f);
    return strtod(buf, nullptr);
}

}  // namespace
