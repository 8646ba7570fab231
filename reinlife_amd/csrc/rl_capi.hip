// rl_capi.hip -- extern "C" surface of libreinlife_hip.so (see include/reinlife_hip.h for the contract).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "rl_common.h"

// implemented in rl_world.hip / rl_policy.hip / rl_render.hip / rl_learn.hip / rl_learn_dueling.hip / rl_learn_prio.hip / rl_learn_td.hip / rl_learn_merge.hip / rl_learn_wide.hip / rl_learn_dueling_wide.hip (also rl_learn_prioritized_wide) / rl_learn_ppo_wide.hip / rl_learn_td_wide.hip
size_t rl_world_smem_bytes(int cpad, int cap, int hash, int plane_stride, int height);
int rl_world_block();
int rl_world_launch_step(rl_world*, const int8_t*, const rl_tape*, const rl_step_out*, hipStream_t);
int rl_world_launch_step_split(rl_world*, const int8_t*, const rl_step_out*, int32_t*, hipStream_t);
int rl_world_launch_step_food(rl_world*, const rl_tape*, float*, hipStream_t);
int rl_world_launch_update(rl_world*, const rl_tape*, const rl_update_out*, hipStream_t);
int rl_world_launch_tick(rl_world*, const int8_t*, const rl_tape*, const rl_step_out*, const rl_update_out*, int, int, int32_t*, hipStream_t);
int rl_world_launch_observe(const rl_world*, float*, hipStream_t);
int rl_world_launch_reset(rl_world*, int, int, float*, int32_t*, int, hipStream_t);
int rl_world_launch_capture(rl_world*, const float*, const int8_t*, const float*, const rl_step_out*, const rl_replay*, int, hipStream_t);
int rl_world_run_supported(const rl_world*, const rl_brain*, int);
int rl_world_launch_run(rl_world*, const rl_brain*, int, int, int8_t*, const rl_step_out*, float* const*, int, int16_t*, int, int, int32_t*, const float*, int, int, const rl_replay*, float*, hipStream_t);
int64_t rl_policy_n_params_impl(int);
int64_t rl_policy_packed_floats_impl(int);
int rl_policy_pack_impl(int, const float*, float*);
int rl_policy_forward_impl(int, const float*, const float*, int64_t, float*, hipStream_t);
size_t rl_policy_work_bytes_impl(const rl_world*);
int rl_policy_act_impl(rl_world*, const rl_brain*, int, const float*, int8_t*, float*, void*, hipStream_t);
int rl_render_launch(rl_world*, const rl_render_style*, const int32_t*, int, uint8_t*, hipStream_t);
int rl_learn_supported_impl(int);
int rl_learn_launch(rl_world*, const rl_learner*, const rl_replay*, int, int, const int32_t*, hipStream_t);
int rl_learn_draw_launch(rl_world*, const rl_learner*, const rl_replay*, int, int, unsigned long long* const*, int32_t*, hipStream_t);
int rl_learn_wide_supported_impl(int);
size_t rl_learn_wide_work_bytes_impl(int);
int rl_learn_wide_launch(rl_world*, const rl_learner*, const rl_replay*, int, int, const int32_t*, void* const*, hipStream_t);
size_t rl_learn_draw_rank_work_bytes_impl(long long);
int rl_learn_draw_rank_launch(rl_world*, const rl_learner*, const rl_replay*, int, int, unsigned long long* const*, int32_t* const*, void* const*, int32_t*, hipStream_t);
size_t rl_learn_prio_draw_rank_work_bytes_impl(long long);
int rl_learn_prioritized_draw_rank_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_prio*, int, int, int, int32_t* const*, double* const*, void* const*, int32_t*, hipStream_t);
int rl_learn_td_draw_rank_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_tdprio*, int, int, int, int32_t* const*, double* const*, void* const*, int32_t*, hipStream_t);
int rl_learn_dueling_wide_supported_impl(int);
size_t rl_learn_dueling_wide_work_bytes_impl(int);
int rl_learn_dueling_wide_launch(rl_world*, const rl_learner*, const rl_replay*, int, int, const int32_t*, void* const*, hipStream_t);
int rl_learn_dueling_supported_impl(int);
int rl_learn_dueling_launch(rl_world*, const rl_learner*, const rl_replay*, int, int, const int32_t*, hipStream_t);
int rl_learn_prioritized_supported_impl(int);
int rl_learn_prioritized_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_prio*, int, int, const int32_t*, hipStream_t);
int rl_learn_prioritized_draw_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_prio*, int, int, int32_t*, hipStream_t);
int rl_learn_prioritized_wide_supported_impl(int);
int rl_learn_prioritized_wide_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_prio*, int, int, const int32_t*, void* const*, hipStream_t);
int rl_learn_prioritized_wide_draw_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_prio*, int, int, int32_t*, hipStream_t);
int rl_learn_td_supported_impl(int);
int rl_learn_td_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_tdprio*, int, int, const int32_t*, hipStream_t);
int rl_learn_td_draw_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_tdprio*, int, int, int32_t*, hipStream_t);
int rl_learn_td_stamp_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_tdprio*, int, hipStream_t);
int rl_learn_td_wide_supported_impl(int);
size_t rl_learn_td_wide_work_bytes_impl(int);
int rl_learn_td_wide_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_tdprio*, int, int, const int32_t*, void* const*, hipStream_t);
int rl_learn_td_wide_draw_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_tdprio*, int, int, int32_t*, hipStream_t);
int rl_learn_td_wide_draw_rank_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_tdprio*, int, int, int, int32_t* const*, double* const*, void* const*, int32_t*, hipStream_t);
int rl_learn_ppo_supported_impl(int);
int rl_learn_ppo_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_ppo*, int, int, const int32_t*, hipStream_t);
int rl_learn_rollout_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_ppo*, int, int, int32_t*, hipStream_t);
int rl_learn_ppo_wide_supported_impl(int);
size_t rl_learn_ppo_wide_work_bytes_impl(int);
int rl_learn_ppo_wide_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_ppo*, int, int, const int32_t*, void* const*, hipStream_t);
int rl_learn_rollout_wide_launch(rl_world*, const rl_learner*, const rl_replay*, const rl_ppo*, int, int, int32_t*, hipStream_t);
int64_t rl_learn_merge_floats_impl(int);
int rl_learn_export_launch(rl_world*, const rl_learner*, int, float*, hipStream_t);
int rl_learn_merge_launch(rl_world*, const rl_learner*, int, const float*, int, int64_t, hipStream_t);
int rl_policy_pack_device_launch(int, const float*, float*, hipStream_t);

static thread_local char g_err[512] = "";

// ---- options: environment read once, rl_set_option afterwards -------------------------------------------------------------------
#include <stdlib.h>
static int parse_variant(const char* v)
{
    if (!v || !*v || !strcmp(v, "auto")) return RL_PV_AUTO;
    if (!strcmp(v, "wave")) return RL_PV_WAVE;
    if (!strcmp(v, "dense")) return RL_PV_DENSE;
    if (!strcmp(v, "pair")) return RL_PV_PAIR;
    return -1;
}
static int parse_block(const char* v)
{
    const int b = (v && *v) ? atoi(v) : 0;
    return (b == 0 || b == 256 || b == 512 || b == 1024) ? b : -1;
}
static rl_options options_from_env()
{
    rl_options o{};
    const int b = parse_block(getenv("RL_WORLD_BLOCK"));
    o.world_block = b < 0 ? 0 : b;
    o.world_generic = getenv("RL_WORLD_GENERIC") ? 1 : 0;
    const int v = parse_variant(getenv("RL_POLICY_VARIANT"));
    o.policy_variant = v < 0 ? RL_PV_AUTO : v;
    o.run_always = getenv("RL_RUN_ALWAYS") ? 1 : 0;
    return o;
}
static rl_options& options_mut()
{
    static rl_options o = options_from_env();   // (thread-safe one-time initialisation)
    return o;
}
const rl_options& rl_options_current() { return options_mut(); }

// The device a handle's buffers live on (taken from the state pointers in rl_bind_state).  Every launching entry point
// makes it current for the duration of the call, so a caller whose current device is another GPU (several handles on
// several GPUs in one process) still launches in the right context.
static int device_of_pointer(const void* p)
{
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged ? a.device : -1;
}
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        int cur = -1;
        if (dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

void rl_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" {

int rl_set_option(const char* name, const char* value)
{
    if (!name) { rl_set_error("rl_set_option: null name"); return RL_E_INVALID; }
    rl_options& o = options_mut();
    const rl_options env = options_from_env();   // value == NULL: back to what the environment says
    if (!strcmp(name, "world_block")) {
        const int b = value ? parse_block(value) : env.world_block;
        if (b < 0) { rl_set_error("rl_set_option: world_block must be 0 (auto), 256, 512 or 1024"); return RL_E_INVALID; }
        o.world_block = b;
    } else if (!strcmp(name, "world_generic")) o.world_generic = value ? (atoi(value) != 0) : env.world_generic;
    else if (!strcmp(name, "policy_variant")) {
        const int v = value ? parse_variant(value) : env.policy_variant;
        if (v < 0) { rl_set_error("rl_set_option: policy_variant must be auto, pair, dense or wave"); return RL_E_INVALID; }
        o.policy_variant = v;
    } else if (!strcmp(name, "run_always")) o.run_always = value ? (atoi(value) != 0) : env.run_always;
    else { rl_set_error("rl_set_option: unknown option '%s'", name); return RL_E_INVALID; }
    return RL_OK;
}

int rl_get_option(const rl_world* h, const char* name)
{
    const rl_options& o = h ? h->opt : rl_options_current();
    if (!name) return -1;
    if (!strcmp(name, "world_block")) return o.world_block;
    if (!strcmp(name, "world_generic")) return o.world_generic;
    if (!strcmp(name, "policy_variant")) return o.policy_variant;
    if (!strcmp(name, "run_always")) return o.run_always;
    return -1;
}

const char* rl_last_error(void) { return g_err; }
const char* rl_version(void) { return "reinlife_hip 0.2 (gfx950)"; }

int rl_create(const rl_config* cfg, rl_world** out)
{
    if (!cfg || !out) { rl_set_error("rl_create: null argument"); return RL_E_INVALID; }
    *out = nullptr;
    if (cfg->width < 3 || cfg->height < 3 || cfg->width > 255 || cfg->height > 255) {  // Grid asserts >= 3 (grid.py:23-24)
        rl_set_error("rl_create: width/height must be in [3,255] (got %dx%d): the reference's Grid needs >= 3 (grid.py:23-24) and has no upper bound; "
                     "this library keeps a world in ONE workgroup's LDS with 8-bit coordinates", cfg->width, cfg->height);
        return RL_E_INVALID;
    }
    const int cells = cfg->width * cfg->height;
    if (cells > RL_MAX_CELLS) {
        rl_set_error("rl_create: %dx%d = %d cells, this library supports width*height <= %d (a world lives in one workgroup's 160 KB of LDS); "
                     "the reference's Grid(width, height) is unbounded (grid.py:22-33) -- a LIMIT of this build, not a rule of the reference",
                     cfg->width, cfg->height, cells, RL_MAX_CELLS);
        return RL_E_UNSUPPORTED;
    }
    if (cfg->n_brains < 1 || cfg->n_brains > RL_MAX_BRAINS) { rl_set_error("rl_create: n_brains must be in [1,%d]", RL_MAX_BRAINS); return RL_E_INVALID; }
    if (cfg->n_worlds < 1 || cfg->n_worlds >= (1 << 19)) { rl_set_error("rl_create: n_worlds must be in [1, 2^19)"); return RL_E_INVALID; }
    if (cfg->max_agents < 1) { rl_set_error("rl_create: max_agents must be >= 1"); return RL_E_INVALID; }
    if (cfg->slot_cap < 64 || (cfg->slot_cap & 63) || cfg->slot_cap > 4096 || cfg->slot_cap < 2 * cfg->max_agents + 2) {
        rl_set_error("rl_create: slot_cap must be a multiple of 64 in [max(64, 2*max_agents+2), 4096] (got %d)", cfg->slot_cap);
        return RL_E_INVALID;
    }
    rl_world* h = new (std::nothrow) rl_world();
    if (!h) { rl_set_error("rl_create: out of memory"); return RL_E_INVALID; }
    h->cfg = *cfg;
    h->opt = rl_options_current();   // the handle's kernels are chosen from this snapshot: nothing reads the environment at a launch
    h->cells = cells;
    h->cpad = (cells + 63) & ~63;
    int hs = 64;
    while (hs < 2 * cfg->slot_cap) hs <<= 1;
    h->hash_size = hs;
    h->smem_bytes = rl_world_smem_bytes(h->cpad, cfg->slot_cap, hs, cfg->width, cfg->height);
    h->block = rl_world_block();
    if (h->smem_bytes > 160 * 1024) {
        rl_set_error("rl_create: world needs %zu bytes of LDS (> 160 KB)", h->smem_bytes);
        delete h;
        return RL_E_UNSUPPORTED;
    }
    *out = h;  // no device call here: handles can be created (and configs validated) without a GPU
    return RL_OK;
}

void rl_destroy(rl_world* h) { delete h; }

int rl_bind_state(rl_world* h, const rl_state* s)
{
    if (!h || !s) { rl_set_error("rl_bind_state: null argument"); return RL_E_INVALID; }
    const void* const* p = (const void* const*)s;
    for (size_t i = 0; i < sizeof(rl_state) / sizeof(void*); ++i)
        if (!p[i]) { rl_set_error("rl_bind_state: state pointer #%zu is null", i); return RL_E_INVALID; }
    h->st = *s;
    h->device = device_of_pointer(s->cell_type);  // -1 (no guard) when it cannot be determined
    h->bound = 1;
    h->lists_valid = 0;  // the caller may have rewritten the state
    return RL_OK;
}

int rl_bind_error_flag(rl_world* h, int32_t* flag)
{
    if (!h) { rl_set_error("rl_bind_error_flag: null handle"); return RL_E_INVALID; }
    h->err_flag = flag;
    return RL_OK;
}

int rl_bind_phase_profile(rl_world* h, long long* device_stamps, int world)
{
    if (!h) { rl_set_error("rl_bind_phase_profile: null handle"); return RL_E_INVALID; }
    h->prof = device_stamps; h->prof_world = world;
    return RL_OK;
}

int rl_bind_policy_work(rl_world* h, void* work)
{
    if (!h) { rl_set_error("rl_bind_policy_work: null handle"); return RL_E_INVALID; }
    h->work = work; h->lists_valid = 0;
    return RL_OK;
}

#define RL_CHECK_BOUND(fn)                                                              \
    if (!h) { rl_set_error(fn ": null handle"); return RL_E_INVALID; }                 \
    if (!h->bound) { rl_set_error(fn ": rl_bind_state was not called"); return RL_E_UNBOUND; }  \
    DeviceGuard rl_guard_(h->device);

int rl_reset_synthetic(rl_world* h, int n_agents, float* obs, void* stream)
{
    RL_CHECK_BOUND("rl_reset_synthetic")
    if (n_agents < 0 || n_agents > h->cfg.slot_cap || n_agents > h->cells) { rl_set_error("rl_reset_synthetic: bad n_agents %d", n_agents); return RL_E_INVALID; }
    return rl_world_launch_reset(h, n_agents, -1, obs, nullptr, 0, (hipStream_t)stream);
}

int rl_reset_families(rl_world* h, float* obs, void* stream)
{
    RL_CHECK_BOUND("rl_reset_families")
    if (h->cfg.n_brains > h->cells) { rl_set_error("rl_reset_families: %d brains on %d cells", h->cfg.n_brains, h->cells); return RL_E_INVALID; }
    return rl_world_launch_reset(h, h->cfg.n_brains, -1, obs, nullptr, 1, (hipStream_t)stream);
}

int rl_refill(rl_world* h, int threshold, int n_agents, float* obs, int32_t* refill_count, void* stream)
{
    RL_CHECK_BOUND("rl_refill")
    if (threshold < 0 || n_agents < 0 || n_agents > h->cfg.slot_cap || n_agents > h->cells) { rl_set_error("rl_refill: bad arguments"); return RL_E_INVALID; }
    return rl_world_launch_reset(h, n_agents, threshold, obs, refill_count, 0, (hipStream_t)stream);
}

int rl_observe(rl_world* h, float* obs, void* stream)
{
    RL_CHECK_BOUND("rl_observe")
    if (!obs) { rl_set_error("rl_observe: null obs"); return RL_E_INVALID; }
    return rl_world_launch_observe(h, obs, (hipStream_t)stream);
}

static int check_tape(const rl_tape* t, const char* fn)
{
    if (!t || !t->food_k) return RL_OK;
    if (!t->food_u || !t->repro_u || !t->birth_k || !t->produce_u || !t->produce_choice) {
        rl_set_error("%s: a tape must provide all six arrays", fn);
        return RL_E_INVALID;
    }
    return RL_OK;
}

static int check_step_out(const rl_step_out* o, const char* fn)
{
    if (!o) return RL_OK;
    const int n = (o->trk_tick != nullptr) + (o->trk_sum != nullptr) + (o->trk_cnt != nullptr) + (o->trk_pop != nullptr);
    if (n != 0 && n != 4) { rl_set_error("%s: the four tracker pointers must be given together", fn); return RL_E_INVALID; }
    return RL_OK;
}

int rl_step(rl_world* h, const int8_t* actions, const rl_tape* tape, const rl_step_out* out, void* stream)
{
    RL_CHECK_BOUND("rl_step")
    if (int rc = check_step_out(out, "rl_step")) return rc;
    if (!actions) { rl_set_error("rl_step: null actions"); return RL_E_INVALID; }
    if (int rc = check_tape(tape, "rl_step")) return rc;
    return rl_world_launch_step(h, actions, tape, out, (hipStream_t)stream);
}

int rl_step_split(rl_world* h, const int8_t* actions, const rl_step_out* out, int32_t* pre_counts, void* stream)
{
    RL_CHECK_BOUND("rl_step_split")
    if (!actions || !pre_counts) { rl_set_error("rl_step_split: null argument"); return RL_E_INVALID; }
    if (int rc = check_step_out(out, "rl_step_split")) return rc;
    return rl_world_launch_step_split(h, actions, out, pre_counts, (hipStream_t)stream);
}

int rl_step_food(rl_world* h, const rl_tape* tape, float* obs, void* stream)
{
    RL_CHECK_BOUND("rl_step_food")
    if (!tape || !tape->food_k || !tape->food_u) { rl_set_error("rl_step_food: a tape with food_k / food_u is required"); return RL_E_INVALID; }
    return rl_world_launch_step_food(h, tape, obs, (hipStream_t)stream);
}

int rl_update(rl_world* h, const rl_tape* tape, const rl_update_out* out, void* stream)
{
    RL_CHECK_BOUND("rl_update")
    if (int rc = check_tape(tape, "rl_update")) return rc;
    return rl_world_launch_update(h, tape, out, (hipStream_t)stream);
}

int rl_tick(rl_world* h, const int8_t* actions, const rl_tape* tape, const rl_step_out* sout, const rl_update_out* uout, void* stream)
{
    RL_CHECK_BOUND("rl_tick")
    if (!actions) { rl_set_error("rl_tick: null actions"); return RL_E_INVALID; }
    if (int rc = check_tape(tape, "rl_tick")) return rc;
    if (int rc = check_step_out(sout, "rl_tick")) return rc;
    return rl_world_launch_tick(h, actions, tape, sout, uout, -1, 0, nullptr, (hipStream_t)stream);
}

int rl_tick_refill(rl_world* h, const int8_t* actions, const rl_step_out* sout, const rl_update_out* uout, int threshold,
                   int n_agents, int32_t* refill_count, void* stream)
{
    RL_CHECK_BOUND("rl_tick_refill")
    if (!actions) { rl_set_error("rl_tick_refill: null actions"); return RL_E_INVALID; }
    if (threshold < 0 || n_agents < 0 || n_agents > h->cfg.slot_cap || n_agents > h->cells) { rl_set_error("rl_tick_refill: bad arguments"); return RL_E_INVALID; }
    if (int rc = check_step_out(sout, "rl_tick_refill")) return rc;
    return rl_world_launch_tick(h, actions, nullptr, sout, uout, threshold, n_agents, refill_count, (hipStream_t)stream);
}

int rl_run_supported(const rl_world* h, const rl_brain* brains, int n_brains)
{
    if (!h || !brains) return 0;
    return rl_world_run_supported(h, brains, n_brains);
}

// The rings transition capture appends to (rl_run_ex with `replays`, rl_capture_transitions), checked before anything is launched: complete,
// and no smaller than the most rows ONE tick of all worlds can append to one ring -- n_worlds * slot_cap, the floor of rl_replay
// (include/reinlife_hip.h).  Below it two rows of one tick can map to the same slot, and nothing in either kernel orders their writes.
static int check_capture_rings(const rl_world* h, const rl_replay* replays, int n_brains, const char* who)
{
    const long long floor_rows = (long long)h->cfg.n_worlds * h->cfg.slot_cap;
    for (int i = 0; i < n_brains; ++i) {
        const rl_replay& r = replays[i];
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.age || !r.count || r.capacity < 1) { rl_set_error("%s: replay %d incomplete", who, i); return RL_E_INVALID; }
        if (r.capacity < floor_rows) {
            rl_set_error("%s: replay %d: capacity %lld is below the floor of %lld rows (n_worlds %d x slot_cap %d, the most rows one tick of all worlds can "
                         "append to one ring: a smaller ring would take two rows of one tick in one slot, written in no order)",
                         who, i, (long long)r.capacity, floor_rows, h->cfg.n_worlds, h->cfg.slot_cap);
            return RL_E_INVALID;
        }
    }
    return RL_OK;
}

int rl_run_ex(rl_world* h, const rl_brain* brains, int n_brains, int n_ticks, int8_t* actions, const rl_step_out* sout,
              float* const obs[2], int first_obs, int16_t* update_src, const rl_run_opts* opts, void* stream)
{
    RL_CHECK_BOUND("rl_run")
    const rl_run_opts none = {-1, 0, nullptr, nullptr, 0, 0, nullptr, nullptr};
    if (!opts) opts = &none;
    if (!brains || !actions || !obs || !obs[0] || !obs[1]) { rl_set_error("rl_run: null argument"); return RL_E_INVALID; }
    if (n_brains != h->cfg.n_brains) { rl_set_error("rl_run: n_brains %d != config %d", n_brains, h->cfg.n_brains); return RL_E_INVALID; }
    if (n_ticks < 0 || (first_obs != 0 && first_obs != 1)) { rl_set_error("rl_run: bad n_ticks / first_obs"); return RL_E_INVALID; }
    if (opts->threshold >= 0 && (opts->n_agents < 0 || opts->n_agents > h->cfg.slot_cap || opts->n_agents > h->cells)) { rl_set_error("rl_run: bad refill arguments"); return RL_E_INVALID; }
    if (int rc = check_step_out(sout, "rl_run")) return rc;
    if (opts->replays)
        if (int rc = check_capture_rings(h, opts->replays, n_brains, "rl_run")) return rc;
    for (int b = 0; b < n_brains; ++b)
        if (brains[b].kind < RL_DQN || brains[b].kind > RL_PERDQN || !brains[b].packed) { rl_set_error("rl_run: brain %d invalid", b); return RL_E_INVALID; }
    if (n_ticks == 0) return RL_OK;
    if (opts->eps_schedule_on_host && (!opts->eps_schedule || (int64_t)n_ticks * n_brains > RL_EPS_INLINE_MAX)) {
        rl_set_error("rl_run: eps_schedule_on_host needs a table of at most %d floats (got %lld)", RL_EPS_INLINE_MAX, (long long)n_ticks * n_brains);
        return RL_E_INVALID;
    }
    return rl_world_launch_run(h, brains, n_brains, n_ticks, actions, sout, obs, first_obs, update_src, opts->threshold, opts->n_agents,
                               opts->refill_count, opts->eps_schedule, opts->eps_schedule_on_host, opts->trk_skip_ticks, opts->replays, opts->policy_out, (hipStream_t)stream);
}

int rl_run(rl_world* h, const rl_brain* brains, int n_brains, int n_ticks, int8_t* actions, const rl_step_out* sout,
           float* const obs[2], int first_obs, int16_t* update_src, int threshold, int n_agents, int32_t* refill_count, void* stream)
{
    const rl_run_opts o = {threshold, n_agents, refill_count, nullptr, 0, 0, nullptr, nullptr};
    return rl_run_ex(h, brains, n_brains, n_ticks, actions, sout, obs, first_obs, update_src, &o, stream);
}

int rl_capture_transitions(rl_world* h, const float* state, const int8_t* actions, const float* policy_out, const rl_step_out* step,
                           const rl_replay* replays, int n_brains, void* stream)
{
    RL_CHECK_BOUND("rl_capture_transitions")
    if (!state || !actions || !step || !replays) { rl_set_error("rl_capture_transitions: null argument"); return RL_E_INVALID; }
    if (n_brains != h->cfg.n_brains || n_brains > RL_MAX_CAPTURE_BRAINS) { rl_set_error("rl_capture_transitions: n_brains %d (config %d, max %d)", n_brains, h->cfg.n_brains, RL_MAX_CAPTURE_BRAINS); return RL_E_INVALID; }
    if (!step->reward || !step->done || !step->src || !step->obs || !step->n_post || !step->age || !step->brain) { rl_set_error("rl_capture_transitions: step outputs reward/done/src/obs/n_post/age/brain are required"); return RL_E_INVALID; }
    if (h->cfg.slot_cap > 4096) { rl_set_error("rl_capture_transitions: slot_cap > 4096"); return RL_E_UNSUPPORTED; }
    if (int rc = check_capture_rings(h, replays, n_brains, "rl_capture_transitions")) return rc;
    return rl_world_launch_capture(h, state, actions, policy_out, step, replays, n_brains, (hipStream_t)stream);
}

int64_t rl_policy_n_params(int kind) { return rl_policy_n_params_impl(kind); }
int64_t rl_policy_packed_floats(int kind) { return rl_policy_packed_floats_impl(kind); }

int rl_policy_pack_weights(int kind, const float* sd, float* packed)
{
    if (!sd || !packed) { rl_set_error("rl_policy_pack_weights: null argument"); return RL_E_INVALID; }
    return rl_policy_pack_impl(kind, sd, packed);
}

int rl_policy_forward(int kind, const float* packed, const float* obs, int64_t n_rows, float* out, void* stream)
{
    if (!packed || !obs || !out || n_rows < 0) { rl_set_error("rl_policy_forward: bad argument"); return RL_E_INVALID; }
    if (kind < RL_DQN || kind > RL_PERDQN) { rl_set_error("rl_policy_forward: unknown brain kind %d", kind); return RL_E_INVALID; }
    if (n_rows == 0) return RL_OK;
    DeviceGuard guard(device_of_pointer(obs));
    return rl_policy_forward_impl(kind, packed, obs, n_rows, out, (hipStream_t)stream);
}

size_t rl_policy_work_bytes(const rl_world* h) { return h ? rl_policy_work_bytes_impl(h) : 0; }

int rl_policy_act(rl_world* h, const rl_brain* brains, int n_brains, const float* obs, int8_t* actions, float* out_q, void* work, void* stream)
{
    RL_CHECK_BOUND("rl_policy_act")
    if (!brains || !obs || !actions || !work) { rl_set_error("rl_policy_act: null argument"); return RL_E_INVALID; }
    if (n_brains != h->cfg.n_brains) { rl_set_error("rl_policy_act: n_brains %d != config %d", n_brains, h->cfg.n_brains); return RL_E_INVALID; }
    for (int b = 0; b < n_brains; ++b)
        if (brains[b].kind < RL_DQN || brains[b].kind > RL_PERDQN || !brains[b].packed) { rl_set_error("rl_policy_act: brain %d invalid", b); return RL_E_INVALID; }
    return rl_policy_act_impl(h, brains, n_brains, obs, actions, out_q, work, (hipStream_t)stream);
}

int rl_learn_supported(int kind) { return rl_learn_supported_impl(kind); }

int rl_learn(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots, void* stream)
{
    if (!h) { rl_set_error("rl_learn: null handle"); return RL_E_INVALID; }
    if (!learners || !rings) { rl_set_error("rl_learn: null learners / rings"); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("rl_learn: n_learners must be in [1,%d] (got %d)", RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1) { rl_set_error("rl_learn: n_steps must be >= 1 (got %d)", n_steps); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        if (!rl_learn_supported_impl(l.kind)) { rl_set_error("rl_learn: learner %d has brain kind %d; this library trains RL_DQN (0) only (rl_learn_supported)", i, l.kind); return RL_E_UNSUPPORTED; }
        if (!l.params || !l.target || !l.adam_m || !l.adam_v || !l.state || !l.packed) { rl_set_error("rl_learn: learner %d: params / target / adam_m / adam_v / state / packed must not be null", i); return RL_E_INVALID; }
        if (l.batch < 1 || l.batch > 32) { rl_set_error("rl_learn: learner %d: batch must be in [1,32] (got %d)", i, l.batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.count || r.capacity < 1 || r.capacity > 0x7fffffff) { rl_set_error("rl_learn: replay %d incomplete (state / state_prime / action / reward / done / count, capacity in [1, 2^31))", i); return RL_E_INVALID; }
    }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_launch(h, learners, rings, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_wide_supported(int kind) { return rl_learn_wide_supported_impl(kind); }

size_t rl_learn_wide_work_bytes(int kind, int batch)
{
    if (!rl_learn_wide_supported_impl(kind)) { rl_set_error("rl_learn_wide_work_bytes: brain kind %d; rl_learn_wide trains RL_DQN (0) only (rl_learn_wide_supported)", kind); return 0; }
    if (batch < 1 || batch > RL_LEARN_WIDE_MAX) { rl_set_error("rl_learn_wide_work_bytes: batch must be in [1,%d] (got %d)", RL_LEARN_WIDE_MAX, batch); return 0; }
    return rl_learn_wide_work_bytes_impl(batch);
}

int rl_learn_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
                  void* const* work, void* stream)
{
    if (!h) { rl_set_error("rl_learn_wide: null handle"); return RL_E_INVALID; }
    if (!learners || !rings) { rl_set_error("rl_learn_wide: null learners / rings"); return RL_E_INVALID; }
    if (!work) { rl_set_error("rl_learn_wide: null work"); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("rl_learn_wide: n_learners must be in [1,%d] (got %d)", RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1) { rl_set_error("rl_learn_wide: n_steps must be >= 1 (got %d)", n_steps); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        if (!rl_learn_wide_supported_impl(l.kind)) { rl_set_error("rl_learn_wide: learner %d has brain kind %d; this entry point trains RL_DQN (0) only (rl_learn_wide_supported)", i, l.kind); return RL_E_INVALID; }
        if (!l.params || !l.target || !l.adam_m || !l.adam_v || !l.state || !l.packed) { rl_set_error("rl_learn_wide: learner %d: params / target / adam_m / adam_v / state / packed must not be null", i); return RL_E_INVALID; }
        if (l.batch < 1 || l.batch > RL_LEARN_WIDE_MAX) { rl_set_error("rl_learn_wide: learner %d: batch must be in [1,%d] (got %d)", i, RL_LEARN_WIDE_MAX, l.batch); return RL_E_INVALID; }
        if (l.batch != learners[0].batch) { rl_set_error("rl_learn_wide: learner %d: batch %d differs from learner 0's %d (the learners of a call share one batch)", i, l.batch, learners[0].batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.count || r.capacity < 1 || r.capacity > 0x7fffffff) { rl_set_error("rl_learn_wide: replay %d incomplete (state / state_prime / action / reward / done / count, capacity in [1, 2^31))", i); return RL_E_INVALID; }
        if (!work[i]) { rl_set_error("rl_learn_wide: work[%d] must not be null (rl_learn_wide_work_bytes)", i); return RL_E_INVALID; }
    }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_wide_launch(h, learners, rings, n_learners, n_steps, slots, work, (hipStream_t)stream);
}

int rl_learn_dueling_supported(int kind) { return rl_learn_dueling_supported_impl(kind); }

int rl_learn_dueling(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots, void* stream)
{
    if (!h) { rl_set_error("rl_learn_dueling: null handle"); return RL_E_INVALID; }
    if (!learners || !rings) { rl_set_error("rl_learn_dueling: null learners / rings"); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("rl_learn_dueling: n_learners must be in [1,%d] (got %d)", RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1) { rl_set_error("rl_learn_dueling: n_steps must be >= 1 (got %d)", n_steps); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        if (!rl_learn_dueling_supported_impl(l.kind)) { rl_set_error("rl_learn_dueling: learner %d has brain kind %d; this entry point trains RL_D3QN (1) only (rl_learn_dueling_supported)", i, l.kind); return RL_E_UNSUPPORTED; }
        if (!l.params || !l.target || !l.adam_m || !l.adam_v || !l.state || !l.packed) { rl_set_error("rl_learn_dueling: learner %d: params / target / adam_m / adam_v / state / packed must not be null", i); return RL_E_INVALID; }
        if (l.batch < 1 || l.batch > 64) { rl_set_error("rl_learn_dueling: learner %d: batch must be in [1,64] (got %d)", i, l.batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.count || r.capacity < 1 || r.capacity > 0x7fffffff) { rl_set_error("rl_learn_dueling: replay %d incomplete (state / state_prime / action / reward / done / count, capacity in [1, 2^31))", i); return RL_E_INVALID; }
    }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_dueling_launch(h, learners, rings, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_dueling_wide_supported(int kind) { return rl_learn_dueling_wide_supported_impl(kind); }

size_t rl_learn_dueling_wide_work_bytes(int kind, int batch)
{
    if (!rl_learn_dueling_wide_supported_impl(kind)) { rl_set_error("rl_learn_dueling_wide_work_bytes: brain kind %d; rl_learn_dueling_wide trains RL_D3QN (1) only (rl_learn_dueling_wide_supported)", kind); return 0; }
    if (batch < 1 || batch > RL_LEARN_DUELING_WIDE_MAX) { rl_set_error("rl_learn_dueling_wide_work_bytes: batch must be in [1,%d] (got %d)", RL_LEARN_DUELING_WIDE_MAX, batch); return 0; }
    return rl_learn_dueling_wide_work_bytes_impl(batch);
}

int rl_learn_dueling_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
                          void* const* work, void* stream)
{
    if (!h) { rl_set_error("rl_learn_dueling_wide: null handle"); return RL_E_INVALID; }
    if (!learners || !rings) { rl_set_error("rl_learn_dueling_wide: null learners / rings"); return RL_E_INVALID; }
    if (!work) { rl_set_error("rl_learn_dueling_wide: null work"); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("rl_learn_dueling_wide: n_learners must be in [1,%d] (got %d)", RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1) { rl_set_error("rl_learn_dueling_wide: n_steps must be >= 1 (got %d)", n_steps); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        if (!rl_learn_dueling_wide_supported_impl(l.kind)) { rl_set_error("rl_learn_dueling_wide: learner %d has brain kind %d; this entry point trains RL_D3QN (1) only (rl_learn_dueling_wide_supported; a PERD3QN brain's prioritised memory is not kept here)", i, l.kind); return RL_E_UNSUPPORTED; }
        if (!l.params || !l.target || !l.adam_m || !l.adam_v || !l.state || !l.packed) { rl_set_error("rl_learn_dueling_wide: learner %d: params / target / adam_m / adam_v / state / packed must not be null", i); return RL_E_INVALID; }
        if (l.batch < 1 || l.batch > RL_LEARN_DUELING_WIDE_MAX) { rl_set_error("rl_learn_dueling_wide: learner %d: batch must be in [1,%d] (got %d)", i, RL_LEARN_DUELING_WIDE_MAX, l.batch); return RL_E_INVALID; }
        if (l.batch != learners[0].batch) { rl_set_error("rl_learn_dueling_wide: learner %d: batch %d differs from learner 0's %d (the learners of a call share one batch)", i, l.batch, learners[0].batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.count || r.capacity < 1 || r.capacity > 0x7fffffff) { rl_set_error("rl_learn_dueling_wide: replay %d incomplete (state / state_prime / action / reward / done / count, capacity in [1, 2^31))", i); return RL_E_INVALID; }
        if (!work[i]) { rl_set_error("rl_learn_dueling_wide: work[%d] must not be null (rl_learn_dueling_wide_work_bytes)", i); return RL_E_INVALID; }
    }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_dueling_wide_launch(h, learners, rings, n_learners, n_steps, slots, work, (hipStream_t)stream);
}

int rl_learn_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, unsigned long long* const* keys,
                  int32_t* slots, void* stream)
{
    if (!h) { rl_set_error("rl_learn_draw: null handle"); return RL_E_INVALID; }
    if (!learners || !rings || !keys || !slots) { rl_set_error("rl_learn_draw: null learners / rings / keys / slots"); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("rl_learn_draw: n_learners must be in [1,%d] (got %d)", RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1) { rl_set_error("rl_learn_draw: n_steps must be >= 1 (got %d)", n_steps); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        if (!learners[i].state || !keys[i]) { rl_set_error("rl_learn_draw: learner %d: state / keys must not be null", i); return RL_E_INVALID; }
        if (learners[i].batch < 1 || learners[i].batch > 32) { rl_set_error("rl_learn_draw: learner %d: batch must be in [1,32] (got %d)", i, learners[i].batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.age || !r.count || r.capacity < 1 || r.capacity > 0x7fffffff) { rl_set_error("rl_learn_draw: replay %d incomplete (state / state_prime / action / reward / done / age / count, capacity in [1, 2^31))", i); return RL_E_INVALID; }
    }
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_draw_launch(h, learners, rings, n_learners, n_steps, keys, slots, (hipStream_t)stream);
}

size_t rl_learn_draw_rank_work_bytes(long long capacity)
{
    if (capacity < 1 || capacity > 0x7fffffff) { rl_set_error("rl_learn_draw_rank_work_bytes: capacity must be in [1, 2^31) (got %lld)", capacity); return 0; }
    return rl_learn_draw_rank_work_bytes_impl(capacity);
}

int rl_learn_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps,
                       unsigned long long* const* keys, int32_t* const* order, void* const* work, int32_t* slots, void* stream)
{
    if (!h) { rl_set_error("rl_learn_draw_rank: null handle"); return RL_E_INVALID; }
    if (!learners) { rl_set_error("rl_learn_draw_rank: null learners"); return RL_E_INVALID; }
    if (!rings) { rl_set_error("rl_learn_draw_rank: null rings"); return RL_E_INVALID; }
    if (!keys) { rl_set_error("rl_learn_draw_rank: null keys"); return RL_E_INVALID; }
    if (!order) { rl_set_error("rl_learn_draw_rank: null order"); return RL_E_INVALID; }
    if (!work) { rl_set_error("rl_learn_draw_rank: null work"); return RL_E_INVALID; }
    if (!slots) { rl_set_error("rl_learn_draw_rank: null slots"); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("rl_learn_draw_rank: n_learners must be in [1,%d] (got %d)", RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1) { rl_set_error("rl_learn_draw_rank: n_steps must be >= 1 (got %d)", n_steps); return RL_E_INVALID; }
    long long draws = 0;
    for (int i = 0; i < n_learners; ++i) {
        const rl_replay& r = rings[i];
        if (!learners[i].state) { rl_set_error("rl_learn_draw_rank: learner %d: state must not be null", i); return RL_E_INVALID; }
        if (!keys[i]) { rl_set_error("rl_learn_draw_rank: keys[%d] must not be null", i); return RL_E_INVALID; }
        if (!order[i]) { rl_set_error("rl_learn_draw_rank: order[%d] must not be null", i); return RL_E_INVALID; }
        if (!work[i]) { rl_set_error("rl_learn_draw_rank: work[%d] must not be null (rl_learn_draw_rank_work_bytes)", i); return RL_E_INVALID; }
        if (learners[i].batch < 1 || learners[i].batch > RL_LEARN_WIDE_MAX) { rl_set_error("rl_learn_draw_rank: learner %d: batch must be in [1,%d] (got %d)", i, RL_LEARN_WIDE_MAX, learners[i].batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.age || !r.count || r.capacity < 1 || r.capacity > 0x7fffffff) { rl_set_error("rl_learn_draw_rank: replay %d incomplete (state / state_prime / action / reward / done / age / count, capacity in [1, 2^31))", i); return RL_E_INVALID; }
        draws += (long long)n_steps * learners[i].batch;
    }
    if (draws > 0x7fffffff) { rl_set_error("rl_learn_draw_rank: n_steps times the learners' batches must stay below 2^31 draws (got %lld)", draws); return RL_E_INVALID; }
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_draw_rank_launch(h, learners, rings, n_learners, n_steps, keys, order, work, slots, (hipStream_t)stream);
}

int rl_learn_prioritized_supported(int kind) { return rl_learn_prioritized_supported_impl(kind); }

// what rl_learn_prioritized and rl_learn_prioritized_draw ask of their common arguments (`draw`: the draw also needs the rings' age column
// and the two scratch buffers of rl_prio).  The wide pair (rl_learn_prioritized_wide, rl_learn_prioritized_wide_draw) asks the same with
// its own batch limit, and ONE batch for all learners of a call: `max_batch`, `one_batch`, the name of the *_supported answer and of the draw.
static int check_prioritized(const char* who, bool draw, rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios,
                             int n_learners, int n_steps, const void* slots, int max_batch = 64, bool one_batch = false,
                             const char* supported = "rl_learn_prioritized_supported", const char* drawn_by = "rl_learn_prioritized_draw")
{
    if (!h) { rl_set_error("%s: null handle", who); return RL_E_INVALID; }
    if (!learners || !rings || !prios) { rl_set_error("%s: null learners / rings / prios", who); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("%s: n_learners must be in [1,%d] (got %d)", who, RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1 || n_steps > 65536) { rl_set_error("%s: n_steps must be in [1,65536] (got %d)", who, n_steps); return RL_E_INVALID; }
    if (!slots) {
        if (draw) rl_set_error("%s: slots must not be null", who);
        else rl_set_error("%s: slots must not be null -- the minibatches of a prioritised memory are drawn by %s", who, drawn_by);
        return RL_E_INVALID;
    }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        const rl_prio& p = prios[i];
        if (!rl_learn_prioritized_supported_impl(l.kind)) { rl_set_error("%s: learner %d has brain kind %d; this entry point trains RL_PERD3QN (2) only (%s)", who, i, l.kind, supported); return RL_E_UNSUPPORTED; }
        if (draw) {
            if (!l.state) { rl_set_error("%s: learner %d: state must not be null", who, i); return RL_E_INVALID; }
        } else if (!l.params || !l.target || !l.adam_m || !l.adam_v || !l.state || !l.packed) {
            rl_set_error("%s: learner %d: params / target / adam_m / adam_v / state / packed must not be null", who, i); return RL_E_INVALID;
        }
        if (l.batch < 1 || l.batch > max_batch) { rl_set_error("%s: learner %d: batch must be in [1,%d] (got %d)", who, i, max_batch, l.batch); return RL_E_INVALID; }
        if (one_batch && l.batch != learners[0].batch) { rl_set_error("%s: learner %d: batch %d differs from learner 0's %d (the learners of a call share one batch)", who, i, l.batch, learners[0].batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.count || (draw && !r.age) || r.capacity < 1 || r.capacity > 0x7fffffff) {
            rl_set_error("%s: replay %d incomplete (state / state_prime / action / reward / done / %scount, capacity in [1, 2^31))", who, i, draw ? "age / " : ""); return RL_E_INVALID;
        }
        if (!p.priority || !p.prio_max || !p.seen) { rl_set_error("%s: prio %d: priority / prio_max / seen must not be null", who, i); return RL_E_INVALID; }
        if (draw && (!p.weight || !p.keys)) { rl_set_error("%s: prio %d: weight / keys must not be null", who, i); return RL_E_INVALID; }
        if (!(p.alpha > 0.0f)) { rl_set_error("%s: prio %d: alpha must be > 0 (got %g)", who, i, (double)p.alpha); return RL_E_INVALID; }
    }
    return RL_OK;
}

int rl_learn_prioritized_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, int n_steps,
                              int32_t* slots, void* stream)
{
    if (int rc = check_prioritized("rl_learn_prioritized_draw", true, h, learners, rings, prios, n_learners, n_steps, slots)) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_prioritized_draw_launch(h, learners, rings, prios, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_prioritized(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, int n_steps,
                         const int32_t* slots, void* stream)
{
    if (int rc = check_prioritized("rl_learn_prioritized", false, h, learners, rings, prios, n_learners, n_steps, slots)) return rc;
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_prioritized_launch(h, learners, rings, prios, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_prioritized_wide_supported(int kind) { return rl_learn_prioritized_wide_supported_impl(kind); }

size_t rl_learn_prioritized_wide_work_bytes(int kind, int batch)
{
    if (!rl_learn_prioritized_wide_supported_impl(kind)) { rl_set_error("rl_learn_prioritized_wide_work_bytes: brain kind %d; rl_learn_prioritized_wide trains RL_PERD3QN (2) only (rl_learn_prioritized_wide_supported)", kind); return 0; }
    if (batch < 1 || batch > RL_LEARN_PRIORITIZED_WIDE_MAX) { rl_set_error("rl_learn_prioritized_wide_work_bytes: batch must be in [1,%d] (got %d)", RL_LEARN_PRIORITIZED_WIDE_MAX, batch); return 0; }
    return rl_learn_dueling_wide_work_bytes_impl(batch);   // the work buffer is rl_learn_dueling_wide's
}

int rl_learn_prioritized_wide_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                                   int n_steps, int32_t* slots, void* stream)
{
    if (int rc = check_prioritized("rl_learn_prioritized_wide_draw", true, h, learners, rings, prios, n_learners, n_steps, slots,
                                   RL_LEARN_PRIORITIZED_WIDE_MAX, true, "rl_learn_prioritized_wide_supported", "rl_learn_prioritized_wide_draw")) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_prioritized_wide_draw_launch(h, learners, rings, prios, n_learners, n_steps, slots, (hipStream_t)stream);
}

size_t rl_learn_prio_draw_rank_work_bytes(long long capacity)
{
    if (capacity < 1 || capacity > 0x7fffffff) { rl_set_error("rl_learn_prio_draw_rank_work_bytes: capacity must be in [1, 2^31) (got %lld)", capacity); return 0; }
    return rl_learn_prio_draw_rank_work_bytes_impl(capacity);
}

// what the two prioritised rank draws ask beyond the race draws' checks: order, cum and work, their entries, and the number of draws
static int check_draw_rank_buffers(const char* who, const rl_learner* learners, int n_learners, int n_steps, int32_t* const* order, double* const* cum,
                                   void* const* work)
{
    long long draws = 0;
    for (int i = 0; i < n_learners; ++i) {
        if (!order[i]) { rl_set_error("%s: order[%d] must not be null", who, i); return RL_E_INVALID; }
        if (!cum[i]) { rl_set_error("%s: cum[%d] must not be null", who, i); return RL_E_INVALID; }
        if (!work[i]) { rl_set_error("%s: work[%d] must not be null (rl_learn_prio_draw_rank_work_bytes)", who, i); return RL_E_INVALID; }
        draws += (long long)n_steps * learners[i].batch;
    }
    if (draws > 0x7fffffff) { rl_set_error("%s: n_steps times the learners' batches must stay below 2^31 draws (got %lld)", who, draws); return RL_E_INVALID; }
    return RL_OK;
}

int rl_learn_prioritized_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, int n_steps,
                                   int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots, void* stream)
{
    const char* who = "rl_learn_prioritized_draw_rank";
    if (h && !order) { rl_set_error("%s: null order", who); return RL_E_INVALID; }
    if (h && !cum) { rl_set_error("%s: null cum", who); return RL_E_INVALID; }
    if (h && !work) { rl_set_error("%s: null work", who); return RL_E_INVALID; }
    if (int rc = check_prioritized(who, true, h, learners, rings, prios, n_learners, n_steps, slots, RL_LEARN_PRIORITIZED_WIDE_MAX, false,
                                   "rl_learn_prioritized_wide_supported", who)) return rc;
    if (int rc = check_draw_rank_buffers(who, learners, n_learners, n_steps, order, cum, work)) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_prioritized_draw_rank_launch(h, learners, rings, prios, n_learners, n_steps, stratified, order, cum, work, slots, (hipStream_t)stream);
}

int rl_learn_prioritized_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, int n_steps,
                              const int32_t* slots, void* const* work, void* stream)
{
    if (h && !work) { rl_set_error("rl_learn_prioritized_wide: null work"); return RL_E_INVALID; }
    if (int rc = check_prioritized("rl_learn_prioritized_wide", false, h, learners, rings, prios, n_learners, n_steps, slots,
                                   RL_LEARN_PRIORITIZED_WIDE_MAX, true, "rl_learn_prioritized_wide_supported", "rl_learn_prioritized_wide_draw")) return rc;
    for (int i = 0; i < n_learners; ++i)
        if (!work[i]) { rl_set_error("rl_learn_prioritized_wide: work[%d] must not be null (rl_learn_prioritized_wide_work_bytes)", i); return RL_E_INVALID; }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_prioritized_wide_launch(h, learners, rings, prios, n_learners, n_steps, slots, work, (hipStream_t)stream);
}

int rl_learn_ppo_supported(int kind) { return rl_learn_ppo_supported_impl(kind); }

// what rl_learn_ppo and rl_learn_rollout ask of their common arguments (`draw`: the rollout draw needs the rings' age column and
// seen / fresh / keys of rl_ppo; the update needs the learner's buffers and the rings' prob column).  The wide pair (rl_learn_ppo_wide,
// rl_learn_rollout_wide) asks the same with its own batch limit, and ONE batch for all learners of a call: `max_batch`, `one_batch`, the
// name of the *_supported answer and of the draw.
static int check_ppo(const char* who, bool draw, rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos,
                     int n_learners, int n_steps, const void* slots, int max_batch = RL_PPO_ROLLOUT_MAX, bool one_batch = false,
                     const char* supported = "rl_learn_ppo_supported", const char* drawn_by = "rl_learn_rollout")
{
    if (!h) { rl_set_error("%s: null handle", who); return RL_E_INVALID; }
    if (!learners || !rings || !ppos) { rl_set_error("%s: null learners / rings / ppos", who); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("%s: n_learners must be in [1,%d] (got %d)", who, RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1 || n_steps > 65536) { rl_set_error("%s: n_steps must be in [1,65536] (got %d)", who, n_steps); return RL_E_INVALID; }
    if (!slots) {
        if (draw) rl_set_error("%s: slots must not be null", who);
        else rl_set_error("%s: slots must not be null -- the rows of a rollout are drawn by %s (or named by the caller)", who, drawn_by);
        return RL_E_INVALID;
    }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        const rl_ppo& p = ppos[i];
        if (!rl_learn_ppo_supported_impl(l.kind)) { rl_set_error("%s: learner %d has brain kind %d; this entry point trains RL_PPO (3) only (%s)", who, i, l.kind, supported); return RL_E_UNSUPPORTED; }
        if (draw) {
            if (!l.state) { rl_set_error("%s: learner %d: state must not be null", who, i); return RL_E_INVALID; }
        } else if (!l.params || !l.adam_m || !l.adam_v || !l.state || !l.packed) {
            rl_set_error("%s: learner %d: params / adam_m / adam_v / state / packed must not be null", who, i); return RL_E_INVALID;
        }
        if (l.batch < 1 || l.batch > max_batch) { rl_set_error("%s: learner %d: batch (the rows of a rollout) must be in [1,%d] (got %d)", who, i, max_batch, l.batch); return RL_E_INVALID; }
        if (one_batch && l.batch != learners[0].batch) { rl_set_error("%s: learner %d: batch %d differs from learner 0's %d (the learners of a call share one batch)", who, i, l.batch, learners[0].batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.count || (draw && !r.age) || r.capacity < 1 || r.capacity > 0x7fffffff) {
            rl_set_error("%s: replay %d incomplete (state / state_prime / action / reward / done / %scount, capacity in [1, 2^31))", who, i, draw ? "age / " : ""); return RL_E_INVALID;
        }
        if (draw) {
            if (!p.seen || !p.fresh || !p.keys) { rl_set_error("%s: ppo %d: seen / fresh / keys must not be null", who, i); return RL_E_INVALID; }
        } else {
            if (!r.prob) { rl_set_error("%s: replay %d has no prob column: a PPO brain's ring records the acting probability (rl_run_opts.policy_out)", who, i); return RL_E_INVALID; }
            if (p.k_epoch < 1 || p.k_epoch > 8) { rl_set_error("%s: ppo %d: k_epoch must be in [1,8] (got %d)", who, i, p.k_epoch); return RL_E_INVALID; }
            if (!(p.eps_clip >= 0.0f) || !(p.lmbda >= 0.0f)) { rl_set_error("%s: ppo %d: lmbda and eps_clip must be >= 0 (got %g, %g)", who, i, (double)p.lmbda, (double)p.eps_clip); return RL_E_INVALID; }
        }
    }
    return RL_OK;
}

int rl_learn_ppo(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                 const int32_t* slots, void* stream)
{
    if (int rc = check_ppo("rl_learn_ppo", false, h, learners, rings, ppos, n_learners, n_steps, slots)) return rc;
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_ppo_launch(h, learners, rings, ppos, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_rollout(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                     int32_t* slots, void* stream)
{
    if (int rc = check_ppo("rl_learn_rollout", true, h, learners, rings, ppos, n_learners, n_steps, slots)) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_rollout_launch(h, learners, rings, ppos, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_ppo_wide_supported(int kind) { return rl_learn_ppo_wide_supported_impl(kind); }

size_t rl_learn_ppo_wide_work_bytes(int kind, int batch)
{
    if (!rl_learn_ppo_wide_supported_impl(kind)) { rl_set_error("rl_learn_ppo_wide_work_bytes: brain kind %d; rl_learn_ppo_wide trains RL_PPO (3) only (rl_learn_ppo_wide_supported)", kind); return 0; }
    if (batch < 1 || batch > RL_LEARN_PPO_WIDE_MAX) { rl_set_error("rl_learn_ppo_wide_work_bytes: batch must be in [1,%d] (got %d)", RL_LEARN_PPO_WIDE_MAX, batch); return 0; }
    return rl_learn_ppo_wide_work_bytes_impl(batch);
}

int rl_learn_rollout_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                          int32_t* slots, void* stream)
{
    if (int rc = check_ppo("rl_learn_rollout_wide", true, h, learners, rings, ppos, n_learners, n_steps, slots, RL_LEARN_PPO_WIDE_MAX, true,
                           "rl_learn_ppo_wide_supported", "rl_learn_rollout_wide")) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_rollout_wide_launch(h, learners, rings, ppos, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_ppo_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                      const int32_t* slots, void* const* work, void* stream)
{
    if (h && !work) { rl_set_error("rl_learn_ppo_wide: null work"); return RL_E_INVALID; }
    if (int rc = check_ppo("rl_learn_ppo_wide", false, h, learners, rings, ppos, n_learners, n_steps, slots, RL_LEARN_PPO_WIDE_MAX, true,
                           "rl_learn_ppo_wide_supported", "rl_learn_rollout_wide")) return rc;
    for (int i = 0; i < n_learners; ++i)
        if (!work[i]) { rl_set_error("rl_learn_ppo_wide: work[%d] must not be null (rl_learn_ppo_wide_work_bytes)", i); return RL_E_INVALID; }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_ppo_wide_launch(h, learners, rings, ppos, n_learners, n_steps, slots, work, (hipStream_t)stream);
}

int rl_render(rl_world* h, const rl_render_style* style, const int32_t* worlds, int n_frames, uint8_t* frames, void* stream)
{
    RL_CHECK_BOUND("rl_render")
    if (!style) { rl_set_error("rl_render: null style"); return RL_E_INVALID; }
    if (!frames) { rl_set_error("rl_render: null frames"); return RL_E_INVALID; }
    if (!style->colors) { rl_set_error("rl_render: style->colors is null"); return RL_E_INVALID; }
    if (!style->tiles) { rl_set_error("rl_render: style->tiles is null"); return RL_E_INVALID; }
    if (style->grid_size < 1 || style->grid_size > 64) { rl_set_error("rl_render: style->grid_size must be in [1,64] (got %d)", style->grid_size); return RL_E_INVALID; }
    if (style->n_colors < 1) { rl_set_error("rl_render: style->n_colors must be >= 1 (got %d)", style->n_colors); return RL_E_INVALID; }
    if (n_frames < 1) { rl_set_error("rl_render: n_frames must be >= 1 (got %d)", n_frames); return RL_E_INVALID; }
    if (!worlds && n_frames > h->cfg.n_worlds) {
        rl_set_error("rl_render: worlds is null (worlds 0..n_frames-1) but n_frames %d > n_worlds %d", n_frames, h->cfg.n_worlds);
        return RL_E_INVALID;
    }
    return rl_render_launch(h, style, worlds, n_frames, frames, (hipStream_t)stream);
}

int rl_learn_td_supported(int kind) { return rl_learn_td_supported_impl(kind); }

// what rl_learn_td and rl_learn_td_draw ask of their common arguments (`draw`: the draw also needs the rings' age column and the keys
// scratch of rl_tdprio; the update needs the learner's buffers and beta).  The wide entries (rl_learn_td_wide, rl_learn_td_wide_draw,
// rl_learn_td_wide_draw_rank) ask the same with their own batch limit, ONE batch for all learners of a call and n_steps up to 65536:
// `max_batch`, `one_batch`, the name of the *_supported answer and of the draw.
static int check_td(const char* who, bool draw, rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds,
                    int n_learners, int n_steps, const void* slots, int max_batch = 64, bool one_batch = false,
                    const char* supported = "rl_learn_td_supported", const char* drawn_by = "rl_learn_td_draw")
{
    if (!h) { rl_set_error("%s: null handle", who); return RL_E_INVALID; }
    if (!learners || !rings || !tds) { rl_set_error("%s: null learners / rings / tds", who); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("%s: n_learners must be in [1,%d] (got %d)", who, RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    if (n_steps < 1) { rl_set_error("%s: n_steps must be >= 1 (got %d)", who, n_steps); return RL_E_INVALID; }
    if (one_batch && n_steps > 65536) { rl_set_error("%s: n_steps must be in [1,65536] (got %d)", who, n_steps); return RL_E_INVALID; }
    if (!slots) {
        if (draw) rl_set_error("%s: slots must not be null", who);
        else rl_set_error("%s: slots must not be null -- the minibatches of a prioritised memory are drawn by %s", who, drawn_by);
        return RL_E_INVALID;
    }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        const rl_tdprio& p = tds[i];
        if (!rl_learn_td_supported_impl(l.kind)) { rl_set_error("%s: learner %d has brain kind %d; this entry point trains RL_PERDQN (4) only (%s)", who, i, l.kind, supported); return RL_E_UNSUPPORTED; }
        if (draw) {
            if (!l.state) { rl_set_error("%s: learner %d: state must not be null", who, i); return RL_E_INVALID; }
        } else if (!l.params || !l.target || !l.adam_m || !l.adam_v || !l.state || !l.packed) {
            rl_set_error("%s: learner %d: params / target / adam_m / adam_v / state / packed must not be null", who, i); return RL_E_INVALID;
        }
        if (l.batch < 1 || l.batch > max_batch) { rl_set_error("%s: learner %d: batch must be in [1,%d] (got %d)", who, i, max_batch, l.batch); return RL_E_INVALID; }
        if (one_batch && l.batch != learners[0].batch) { rl_set_error("%s: learner %d: batch %d differs from learner 0's %d (the learners of a call share one batch)", who, i, l.batch, learners[0].batch); return RL_E_INVALID; }
        if (!r.state || !r.state_prime || !r.action || !r.reward || !r.done || !r.count || (draw && !r.age) || r.capacity < 1 || r.capacity > 0x7fffffff) {
            rl_set_error("%s: replay %d incomplete (state / state_prime / action / reward / done / %scount, capacity in [1, 2^31))", who, i, draw ? "age / " : ""); return RL_E_INVALID;
        }
        if (draw) {
            if (!p.priority || !p.keys || !p.seen) { rl_set_error("%s: td %d: priority / keys / seen must not be null", who, i); return RL_E_INVALID; }
        } else {
            if (!p.priority || !p.seen || !p.beta) { rl_set_error("%s: td %d: priority / seen / beta must not be null", who, i); return RL_E_INVALID; }
            if (!(p.prio_a > 0.0f)) { rl_set_error("%s: td %d: prio_a must be > 0 (got %g)", who, i, (double)p.prio_a); return RL_E_INVALID; }
        }
    }
    return RL_OK;
}

int rl_learn_td_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                     int32_t* slots, void* stream)
{
    if (int rc = check_td("rl_learn_td_draw", true, h, learners, rings, tds, n_learners, n_steps, slots)) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_td_draw_launch(h, learners, rings, tds, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_td_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                          int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots, void* stream)
{
    const char* who = "rl_learn_td_draw_rank";
    if (h && !order) { rl_set_error("%s: null order", who); return RL_E_INVALID; }
    if (h && !cum) { rl_set_error("%s: null cum", who); return RL_E_INVALID; }
    if (h && !work) { rl_set_error("%s: null work", who); return RL_E_INVALID; }
    if (int rc = check_td(who, true, h, learners, rings, tds, n_learners, n_steps, slots)) return rc;
    if (int rc = check_draw_rank_buffers(who, learners, n_learners, n_steps, order, cum, work)) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_td_draw_rank_launch(h, learners, rings, tds, n_learners, n_steps, stratified, order, cum, work, slots, (hipStream_t)stream);
}

int rl_learn_td(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                const int32_t* slots, void* stream)
{
    if (int rc = check_td("rl_learn_td", false, h, learners, rings, tds, n_learners, n_steps, slots)) return rc;
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_td_launch(h, learners, rings, tds, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_td_wide_supported(int kind) { return rl_learn_td_wide_supported_impl(kind); }

size_t rl_learn_td_wide_work_bytes(int kind, int batch)
{
    if (!rl_learn_td_wide_supported_impl(kind)) { rl_set_error("rl_learn_td_wide_work_bytes: brain kind %d; rl_learn_td_wide trains RL_PERDQN (4) only (rl_learn_td_wide_supported)", kind); return 0; }
    if (batch < 1 || batch > RL_LEARN_TD_WIDE_MAX) { rl_set_error("rl_learn_td_wide_work_bytes: batch must be in [1,%d] (got %d)", RL_LEARN_TD_WIDE_MAX, batch); return 0; }
    return rl_learn_td_wide_work_bytes_impl(batch);
}

int rl_learn_td_wide_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                          int32_t* slots, void* stream)
{
    if (int rc = check_td("rl_learn_td_wide_draw", true, h, learners, rings, tds, n_learners, n_steps, slots, RL_LEARN_TD_WIDE_MAX, true,
                          "rl_learn_td_wide_supported", "rl_learn_td_wide_draw")) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_td_wide_draw_launch(h, learners, rings, tds, n_learners, n_steps, slots, (hipStream_t)stream);
}

int rl_learn_td_wide_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                               int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots, void* stream)
{
    const char* who = "rl_learn_td_wide_draw_rank";
    if (h && !order) { rl_set_error("%s: null order", who); return RL_E_INVALID; }
    if (h && !cum) { rl_set_error("%s: null cum", who); return RL_E_INVALID; }
    if (h && !work) { rl_set_error("%s: null work", who); return RL_E_INVALID; }
    if (int rc = check_td(who, true, h, learners, rings, tds, n_learners, n_steps, slots, RL_LEARN_TD_WIDE_MAX, true,
                          "rl_learn_td_wide_supported", who)) return rc;
    if (int rc = check_draw_rank_buffers(who, learners, n_learners, n_steps, order, cum, work)) return rc;
    DeviceGuard guard(device_of_pointer(slots));
    return rl_learn_td_wide_draw_rank_launch(h, learners, rings, tds, n_learners, n_steps, stratified, order, cum, work, slots, (hipStream_t)stream);
}

int rl_learn_td_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                     const int32_t* slots, void* const* work, void* stream)
{
    if (h && !work) { rl_set_error("rl_learn_td_wide: null work"); return RL_E_INVALID; }
    if (int rc = check_td("rl_learn_td_wide", false, h, learners, rings, tds, n_learners, n_steps, slots, RL_LEARN_TD_WIDE_MAX, true,
                          "rl_learn_td_wide_supported", "rl_learn_td_wide_draw")) return rc;
    for (int i = 0; i < n_learners; ++i)
        if (!work[i]) { rl_set_error("rl_learn_td_wide: work[%d] must not be null (rl_learn_td_wide_work_bytes)", i); return RL_E_INVALID; }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_td_wide_launch(h, learners, rings, tds, n_learners, n_steps, slots, work, (hipStream_t)stream);
}

// rl_learn_td_stamp reads neither batch, min_size, keys, beta nor p_new: its own check, argument by argument
int rl_learn_td_stamp(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, void* stream)
{
    const char* who = "rl_learn_td_stamp";
    if (!h) { rl_set_error("%s: null handle", who); return RL_E_INVALID; }
    if (!learners) { rl_set_error("%s: null learners", who); return RL_E_INVALID; }
    if (!rings) { rl_set_error("%s: null rings", who); return RL_E_INVALID; }
    if (!tds) { rl_set_error("%s: null tds", who); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("%s: n_learners must be in [1,%d] (got %d)", who, RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const rl_replay& r = rings[i];
        const rl_tdprio& p = tds[i];
        if (!rl_learn_td_supported_impl(l.kind)) { rl_set_error("%s: learner %d has brain kind %d; this entry point stamps RL_PERDQN (4) memories only (rl_learn_td_supported)", who, i, l.kind); return RL_E_UNSUPPORTED; }
        if (!l.params) { rl_set_error("%s: learner %d: params must not be null", who, i); return RL_E_INVALID; }
        if (!l.target) { rl_set_error("%s: learner %d: target must not be null", who, i); return RL_E_INVALID; }
        const void* cols[6] = {r.state, r.state_prime, r.action, r.reward, r.done, r.count};
        static const char* const names[6] = {"state", "state_prime", "action", "reward", "done", "count"};
        for (int c = 0; c < 6; ++c)
            if (!cols[c]) { rl_set_error("%s: replay %d: %s must not be null", who, i, names[c]); return RL_E_INVALID; }
        if (r.capacity < 1 || r.capacity > 0x7fffffff) { rl_set_error("%s: replay %d: capacity must be in [1, 2^31) (got %lld)", who, i, (long long)r.capacity); return RL_E_INVALID; }
        if (!p.priority) { rl_set_error("%s: td %d: priority must not be null", who, i); return RL_E_INVALID; }
        if (!p.seen) { rl_set_error("%s: td %d: seen must not be null", who, i); return RL_E_INVALID; }
        if (!(p.prio_a > 0.0f)) { rl_set_error("%s: td %d: prio_a must be > 0 (got %g)", who, i, (double)p.prio_a); return RL_E_INVALID; }
    }
    DeviceGuard guard(device_of_pointer(tds[0].priority));
    return rl_learn_td_stamp_launch(h, learners, rings, tds, n_learners, (hipStream_t)stream);
}

int64_t rl_learn_merge_floats(int kind) { return rl_learn_merge_floats_impl(kind); }

// what rl_learn_export and rl_learn_merge ask of their common arguments (`merge`: the merge also writes target and packed); *total: the
// floats of the learners' segments laid end to end
static int check_merge(const char* who, bool merge, rl_world* h, const rl_learner* learners, int n_learners, int64_t* total)
{
    if (!h) { rl_set_error("%s: null handle", who); return RL_E_INVALID; }
    if (!learners) { rl_set_error("%s: null learners", who); return RL_E_INVALID; }
    if (n_learners < 1 || n_learners > RL_MAX_CAPTURE_BRAINS) { rl_set_error("%s: n_learners must be in [1,%d] (got %d)", who, RL_MAX_CAPTURE_BRAINS, n_learners); return RL_E_INVALID; }
    *total = 0;
    for (int i = 0; i < n_learners; ++i) {
        const rl_learner& l = learners[i];
        const int64_t seg = rl_learn_merge_floats_impl(l.kind);
        if (seg < 0) { rl_set_error("%s: learner %d has brain kind %d; no learner of this library has that kind (RL_DQN 0 .. RL_PERDQN 4)", who, i, l.kind); return RL_E_UNSUPPORTED; }
        if (!l.params || !l.adam_m || !l.adam_v || !l.state) { rl_set_error("%s: learner %d: params / adam_m / adam_v / state must not be null", who, i); return RL_E_INVALID; }
        if (merge && !l.packed) { rl_set_error("%s: learner %d: packed must not be null", who, i); return RL_E_INVALID; }
        if (merge && !l.target && l.kind != RL_PPO) { rl_set_error("%s: learner %d: target must not be null (only an RL_PPO learner has none)", who, i); return RL_E_INVALID; }
        *total += seg;
    }
    return RL_OK;
}

int rl_learn_export(rl_world* h, const rl_learner* learners, int n_learners, float* row, void* stream)
{
    int64_t total;
    if (int rc = check_merge("rl_learn_export", false, h, learners, n_learners, &total)) return rc;
    if (!row) { rl_set_error("rl_learn_export: null row (learners 0..%d need %lld floats)", n_learners - 1, (long long)total); return RL_E_INVALID; }
    DeviceGuard guard(device_of_pointer(row));
    return rl_learn_export_launch(h, learners, n_learners, row, (hipStream_t)stream);
}

int rl_learn_merge(rl_world* h, const rl_learner* learners, int n_learners, const float* rows, int n_ranks, int64_t row_stride_floats, void* stream)
{
    int64_t total;
    if (int rc = check_merge("rl_learn_merge", true, h, learners, n_learners, &total)) return rc;
    if (!rows) { rl_set_error("rl_learn_merge: null rows (learners 0..%d need %lld floats per rank)", n_learners - 1, (long long)total); return RL_E_INVALID; }
    if (n_ranks < 1 || n_ranks > 64) { rl_set_error("rl_learn_merge: n_ranks must be in [1,64] (got %d; learners 0..%d)", n_ranks, n_learners - 1); return RL_E_INVALID; }
    if (row_stride_floats < total) {
        rl_set_error("rl_learn_merge: row_stride_floats %lld is shorter than the learners' segments: learner %d ends at float %lld", (long long)row_stride_floats, n_learners - 1, (long long)total);
        return RL_E_INVALID;
    }
    DeviceGuard guard(device_of_pointer(learners[0].params));
    return rl_learn_merge_launch(h, learners, n_learners, rows, n_ranks, row_stride_floats, (hipStream_t)stream);
}

int rl_policy_pack_device(int kind, const float* params, float* packed, void* stream)
{
    if (kind < RL_DQN || kind > RL_PERDQN) { rl_set_error("rl_policy_pack_device: unknown brain kind %d", kind); return RL_E_INVALID; }
    if (!params || !packed) { rl_set_error("rl_policy_pack_device: kind %d: params / packed must not be null", kind); return RL_E_INVALID; }
    DeviceGuard guard(device_of_pointer(packed));
    return rl_policy_pack_device_launch(kind, params, packed, (hipStream_t)stream);
}

void rl_philox(uint64_t seed, uint32_t epoch, uint32_t world, uint32_t tick, uint32_t site, uint32_t index, uint32_t out[4])
{
    const rl_u4 r = rl_philox4x32(seed, epoch, world, tick, site, index);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

}  // extern "C"
