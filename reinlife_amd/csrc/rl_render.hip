// rl_render.hip -- k_render: the frames of any set of worlds of a handle painted straight from rl_state into a caller-owned uint8 RGB
// buffer, byte for byte what reinlife_amd/Helpers/render.py::Visualize.frame paints (reference: ReinLife/Helpers/render.py:51-239).
//
// A frame is a pure function of each pixel's cell.  At offset (px, py) inside cell (i, j), the first that applies:
//   1 food square   cell_type is food / poison / super food and (px, py) lies in the square at food_off, side food_size
//   2 eye           the cell has an agent and (px, py) lies in one of the two eye squares (black)
//   3 border        the `border`-pixel frame of the body square (all of it when 2 * border >= body_size): red when the agent killed
//                   this tick, else body * (1 - health / 205) in float64
//   4 body          colors[gene mod n_colors] in the body square at body_off, side body_size
//   5 background    the cell's tile colour
// "the agent of the cell" = the LAST list entry k < n_agents with RL_F_DEAD clear whose (a_i, a_j) is this cell and lies on the grid.
// All geometry arrives as integers computed by the host painter's own expressions; only the border colour is floating point here.
//
// Shape.  The kernel is write-bound.  Grid = (bands of cell rows, frame); a band's pixel rows are ONE contiguous byte range of the
// frame, cut at the 16-byte boundaries of the ABSOLUTE address: a short head and tail go out as byte stores, the rest as aligned
// 16-byte stores.  Phase A: the workgroup scans the world's agent list once, resolves "last entry wins" for its band with an LDS
// atomicMax on the list index, and writes one small LDS record per cell (background + food kind + agent bit, body RGB, border RGB).
// Phase B, two forms:
//   lines    (whenever they fit into LDS) The pixel rows of a cell row differ only by which of the food / eye / body / border row
//            ranges py lies in: the host groups py into classes (6 of 24 rows at grid size 24, 4 of 8 at 8).  The workgroup composes
//            ONE scanline per class and cell row in LDS -- py is uniform there, so the row tests are scalar -- and every 16-byte
//            chunk of the band is then a copy from its row's line: five aligned LDS words funnel-shifted to the chunk's alignment
//            (a chunk that straddles two pixel rows is gathered bytewise).
//   direct   (any shape) units of 48 bytes = three stores per thread; 48 is a multiple of 3, so every unit of a workgroup starts in
//            the same colour channel (three specialisations of the packing), and a thread walks its 16-17 pixels incrementally.
// Nothing outside frames[0 : n_frames * frame_bytes] is touched and rl_state is only read.
#include "rl_common.h"

namespace {

constexpr int kRenderBlock = 256;
constexpr int kRenderMaxBandCells = 1024;   // LDS records of one band (16 KB)
constexpr int kErrRenderWorld = 5;           // error-flag code: world id outside [0, n_worlds) (include/reinlife_hip.h, rl_bind_error_flag)

struct RenderParams {
    const uint8_t* cell_type;    // [R][C]
    const int32_t* n_agents;     // [R]
    const uint8_t* a_i;          // [R][cap]
    const uint8_t* a_j;
    const int32_t* a_health;
    const int32_t* a_gene;
    const uint8_t* a_flags;
    const double* colors;        // [n_colors][3]
    const uint8_t* tiles;        // [H][W][3]
    const int32_t* worlds;       // [n_frames] or null
    uint8_t* frames;
    int32_t* err;
    int W, H, cap, n_worlds, n_colors;
    int gs, body_off, body_size, border, eye_size, eye_y, eye_x0, eye_x1, food_off, food_size;
    int frame0;                  // first frame of this launch (grid.y <= 65535 frames per launch)
    int band_rows;               // cell rows per band (band_rows * W <= kRenderMaxBandCells)
    uint32_t row_bytes;          // W * gs * 3
    uint32_t frame_bytes;        // H * gs * row_bytes  (<= 4096 cells * 64 * 64 * 3 < 2^26)
    int n_cls;                   // > 0: the `lines` form with n_cls scanline classes; 0: the `direct` form
    int line_stride;             // bytes between two lines in LDS: whole groups of 4 pixels (a multiple of 12)
    uint32_t m_gs, m_cls;        // div_small multipliers for grid_size and n_cls
    uint8_t cls_of_py[64];       // class of every pixel row of a cell
    uint8_t rep_py[16];          // a pixel row of every class
};

// record word 0: background RGB | food kind << 24 (0 none, 1 food, 2 poison, 3 super food) | has agent << 26
constexpr uint32_t kRecAgent = 1u << 26;

__device__ inline uint32_t pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// np.clip(x, 0, 255).astype(np.uint8): clip, then truncate
__device__ inline uint32_t clip_u8(double x) { return (uint32_t)(int)fmin(fmax(x, 0.0), 255.0); }

struct Rec { uint32_t bg, body, border; };

// the colour of pixel (px, py) of a cell whose record is r (rules 1-5)
__device__ inline uint32_t pixel_rgb(const RenderParams& p, const Rec& r, int px, int py)
{
    const uint32_t kind = (r.bg >> 24) & 3u;
    if (kind) {
        const unsigned fx = (unsigned)(px - p.food_off), fy = (unsigned)(py - p.food_off);
        if (fx < (unsigned)p.food_size && fy < (unsigned)p.food_size)
            return kind == 1 ? 0xFFFFFFu : kind == 2 ? 0u : 0x0000FFu;
    }
    if (r.bg & kRecAgent) {
        const unsigned ey = (unsigned)(py - p.eye_y);
        if (ey < (unsigned)p.eye_size && ((unsigned)(px - p.eye_x0) < (unsigned)p.eye_size || (unsigned)(px - p.eye_x1) < (unsigned)p.eye_size))
            return 0u;
        const unsigned bx = (unsigned)(px - p.body_off), by = (unsigned)(py - p.body_off);
        const unsigned bs = (unsigned)p.body_size, bw = (unsigned)p.border;
        if (bx < bs && by < bs) {
            if (2 * bw >= bs || bx < bw || by < bw || bx >= bs - bw || by >= bs - bw) return r.border;
            return r.body;
        }
    }
    return r.bg & 0xFFFFFFu;
}

struct Lds {
    int win[kRenderMaxBandCells];
    uint32_t bg[kRenderMaxBandCells], body[kRenderMaxBandCells], border[kRenderMaxBandCells];
    uint8_t cls[64], rep[16];
};
constexpr int kRenderLineBytes = 48 * 1024;   // LDS for the composed lines (dynamic; the records above are 16 KB)

__device__ inline Rec load_rec(const Lds& s, int c) { return Rec{s.bg[c], s.body[c], s.border[c]}; }

// Position of one pixel inside the band: cell row (band-local), cell column, offsets inside the cell.
struct Cursor { int il, j, py, px; };

__device__ inline Cursor cursor_at(const RenderParams& p, uint32_t pixel, uint32_t wpx)
{
    const uint32_t y = pixel / wpx, x = pixel - y * wpx;
    Cursor c;
    c.il = (int)(y / (uint32_t)p.gs); c.py = (int)(y - (uint32_t)c.il * (uint32_t)p.gs);
    c.j = (int)(x / (uint32_t)p.gs);  c.px = (int)(x - (uint32_t)c.j * (uint32_t)p.gs);
    return c;
}

// one byte of the band (band-relative offset o): head and tail of the byte range
__device__ inline uint8_t band_byte(const RenderParams& p, const Lds& s, uint32_t o, uint32_t wpx)
{
    const uint32_t pixel = o / 3u, ch = o - pixel * 3u;
    const Cursor c = cursor_at(p, pixel, wpx);
    return (uint8_t)(pixel_rgb(p, load_rec(s, c.il * p.W + c.j), c.px, c.py) >> (8u * ch));
}

// 48 bytes starting at band-relative offset o, whose first byte is channel C0 of its pixel: NP pixels -> 12 dwords -> three 16-byte stores
template <int C0>
__device__ inline void band_unit(const RenderParams& p, const Lds& s, uint32_t o, uint32_t wpx, uint8_t* dst)
{
    constexpr int NP = C0 ? 17 : 16;
    Cursor c = cursor_at(p, o / 3u, wpx);
    int cell = c.il * p.W + c.j;
    Rec r = load_rec(s, cell);
    uint32_t rgb[17];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        rgb[n] = pixel_rgb(p, r, c.px, c.py);
        if (n + 1 < NP) {   // step to the next pixel of the band (the last pixel of a unit lies inside the band: no step past it)
            if (++c.px == p.gs) {
                c.px = 0; ++cell;
                if (++c.j == p.W) {       // next pixel row: the same cell row unless py wraps
                    c.j = 0;
                    if (++c.py == p.gs) c.py = 0; else cell -= p.W;
                }
                r = load_rec(s, cell);
            }
        }
    }
    if (NP == 16) rgb[16] = 0;
    uint32_t out[12];
#pragma unroll
    for (int d = 0; d < 12; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int sb = 4 * d + e + C0;
            w |= ((rgb[sb / 3] >> (8 * (sb % 3))) & 0xFFu) << (8 * e);
        }
        out[d] = w;
    }
    uint4* q = reinterpret_cast<uint4*>(dst);   // 16-byte aligned by construction
    q[0] = make_uint4(out[0], out[1], out[2], out[3]);
    q[1] = make_uint4(out[4], out[5], out[6], out[7]);
    q[2] = make_uint4(out[8], out[9], out[10], out[11]);
}

// ---- the `lines` form --------------------------------------------------------------------------------------------------------
// line (r, c) = the scanline of cell row r (band-local) for the pixel rows of class c, at lines + (r * n_cls + c) * line_stride
// x / d for 0 <= x < 16384 and 1 <= d <= 64 with m = 2^20 / d + 1 (render_plan): the error of m * d against 2^20 is at most d, and
// x * d < 2^20 (the product x * m needs 35 bits)
__device__ inline uint32_t div_small(uint32_t x, uint32_t m) { return (uint32_t)(((uint64_t)x * m) >> 20); }

__device__ inline void compose_lines(const RenderParams& p, const Lds& s, uint8_t* lines, int rows, int ncells, uint32_t wpx, int tid)
{
    const int groups = (int)((wpx + 3u) / 4u);   // 4 pixels = 12 bytes = 3 words
    const int total = rows * p.n_cls * groups;
    const int dq = kRenderBlock / groups, dr = kRenderBlock - dq * groups;   // a thread's next group: kRenderBlock further on
    int rc = tid / groups, g = tid - rc * groups;
    for (int idx = tid; idx < total; idx += kRenderBlock) {
        const int r = (int)div_small((uint32_t)rc, p.m_cls), py = s.rep[rc - r * p.n_cls];
        uint32_t* const line = reinterpret_cast<uint32_t*>(lines + (size_t)rc * p.line_stride);
        const int x = 4 * g;
        const int j = (int)div_small((uint32_t)x, p.m_gs);
        int px = x - j * p.gs;
        int cell = r * p.W + j;
        Rec rec = load_rec(s, min(cell, ncells - 1));
        uint32_t rgb[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            rgb[n] = (uint32_t)(x + n) < wpx ? pixel_rgb(p, rec, px, py) : 0u;   // (the last group may reach past the row)
            if (n < 3 && ++px == p.gs) { px = 0; ++cell; rec = load_rec(s, min(cell, ncells - 1)); }
        }
        line[3 * g] = rgb[0] | (rgb[1] << 24);
        line[3 * g + 1] = (rgb[1] >> 8) | (rgb[2] << 16);
        line[3 * g + 2] = (rgb[2] >> 16) | (rgb[3] << 8);
        rc += dq; g += dr;
        if (g >= groups) { g -= groups; ++rc; }
    }
}

// where band-relative byte o lives in the lines
__device__ inline const uint8_t* line_byte(const RenderParams& p, const Lds& s, const uint8_t* lines, uint32_t o)
{
    const uint32_t y = o / p.row_bytes, xo = o - y * p.row_bytes;
    const uint32_t r = y / (uint32_t)p.gs, py = y - r * (uint32_t)p.gs;
    return lines + (size_t)(r * (uint32_t)p.n_cls + s.cls[py]) * p.line_stride + xo;
}

// 16 bytes of the band at offset o = y * row_bytes + xo
__device__ inline uint4 line_chunk(const RenderParams& p, const Lds& s, const uint8_t* lines, uint32_t o, uint32_t y, uint32_t xo)
{
    uint32_t d[4];
    if (xo + 16u <= p.row_bytes) {   // inside one pixel row: five aligned words (lines and their stride are word-aligned), shifted
        const uint32_t r = div_small(y, p.m_gs), py = y - r * (uint32_t)p.gs;
        const uint8_t* src = lines + (size_t)(r * (uint32_t)p.n_cls + s.cls[py]) * p.line_stride + (xo & ~3u);
        const uint32_t* a = reinterpret_cast<const uint32_t*>(src);
        const uint32_t sh = (xo & 3u) * 8u;
        const uint32_t w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3], w4 = a[4];   // (a[4]: at most the 16 bytes of padding behind the last line)
        d[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
        d[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
        d[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
        d[3] = (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh);
    } else {                         // the chunk straddles two pixel rows (possibly two cell rows)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w |= (uint32_t)*line_byte(p, s, lines, o + 4 * k + e) << (8 * e);
            d[k] = w;
        }
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

extern __shared__ __attribute__((aligned(16))) uint8_t g_lines[];

__global__ __launch_bounds__(kRenderBlock) void k_render(const RenderParams p)
{
    __shared__ Lds s;
    const int tid = threadIdx.x, f = p.frame0 + (int)blockIdx.y;
    const int w = p.worlds ? p.worlds[f] : f;
    if (w < 0 || w >= p.n_worlds) {   // (uniform over the workgroup) the frame stays as it was
        if (tid == 0 && blockIdx.x == 0 && p.err && atomicCAS(p.err, 0, kErrRenderWorld) == 0) { p.err[1] = w; p.err[2] = f; p.err[3] = 0; }
        return;
    }
    const int i0 = blockIdx.x * p.band_rows;
    const int rows = min(p.band_rows, p.H - i0);
    const int ncells = rows * p.W;

    // ---- phase A: the band's cell records --------------------------------------------------------------------------------------
    for (int c = tid; c < ncells; c += kRenderBlock) s.win[c] = -1;
    if (tid < 64) s.cls[tid] = p.cls_of_py[tid];
    if (tid < 16) s.rep[tid] = p.rep_py[tid];
    __syncthreads();
    const size_t abase = (size_t)w * p.cap;
    const int n = min(max(p.n_agents[w], 0), p.cap);
    for (int k = tid; k < n; k += kRenderBlock) {
        const int ai = p.a_i[abase + k], aj = p.a_j[abase + k];
        if (!(p.a_flags[abase + k] & RL_F_DEAD) && ai >= i0 && ai < i0 + rows && aj < p.W) atomicMax(&s.win[(ai - i0) * p.W + aj], k);
    }
    __syncthreads();
    for (int c = tid; c < ncells; c += kRenderBlock) {
        const int gc = i0 * p.W + c;   // cell index in the world (row-major)
        const uint8_t ct = p.cell_type[(size_t)w * (p.W * p.H) + gc];
        const uint32_t kind = ct == RL_FOOD ? 1u : ct == RL_POISON ? 2u : ct == RL_SUPER_FOOD ? 3u : 0u;
        uint32_t bg = pack_rgb(p.tiles[3 * gc], p.tiles[3 * gc + 1], p.tiles[3 * gc + 2]) | (kind << 24);
        uint32_t body = 0, border = 0;
        const int k = s.win[c];
        if (k >= 0) {
            bg |= kRecAgent;
            const int g = p.a_gene[abase + k];
            const int col = ((g % p.n_colors) + p.n_colors) % p.n_colors;   // Python's %: never negative
            const double cr = p.colors[3 * col], cg = p.colors[3 * col + 1], cb = p.colors[3 * col + 2];
            body = pack_rgb(clip_u8(cr), clip_u8(cg), clip_u8(cb));
            if (p.a_flags[abase + k] & RL_F_KILLED) border = 0x0000FFu;
            else {
                const double t = 1.0 - (double)p.a_health[abase + k] / 205.0;   // render.py:151-152: lerp towards black
                border = pack_rgb(clip_u8(cr * t), clip_u8(cg * t), clip_u8(cb * t));
            }
        }
        s.bg[c] = bg; s.body[c] = body; s.border[c] = border;
    }
    __syncthreads();

    // ---- phase B: the band's bytes ---------------------------------------------------------------------------------------------
    const uint32_t wpx = (uint32_t)(p.W * p.gs);
    const uint32_t len = (uint32_t)(rows * p.gs) * p.row_bytes;
    uint8_t* const dst = p.frames + ((uint64_t)f * p.frame_bytes + (uint64_t)(i0 * p.gs) * p.row_bytes);   // 64-bit byte offsets
    const uint32_t head = min((uint32_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u), len);
    if (p.n_cls > 0) {
        compose_lines(p, s, g_lines, rows, ncells, wpx, tid);
        __syncthreads();
        const uint32_t chunks = (len - head) / 16u, rest0 = head + chunks * 16u;
        for (uint32_t o = tid; o < head + (len - rest0); o += kRenderBlock) {   // (< 16 + 16 bytes)
            const uint32_t b = o < head ? o : rest0 + (o - head);
            dst[b] = *line_byte(p, s, g_lines, b);
        }
        // a thread's chunks lie kRenderBlock * 16 bytes apart: (y, xo) advance by a fixed (dy, dx), one carry at most
        const uint32_t dy = (kRenderBlock * 16u) / p.row_bytes, dx = (kRenderBlock * 16u) - dy * p.row_bytes;
        uint32_t o = head + tid * 16u;
        uint32_t y = o / p.row_bytes, xo = o - y * p.row_bytes;
        for (uint32_t u = tid; u < chunks; u += kRenderBlock) {
            *reinterpret_cast<uint4*>(dst + o) = line_chunk(p, s, g_lines, o, y, xo);
            o += kRenderBlock * 16u; y += dy; xo += dx;
            if (xo >= p.row_bytes) { xo -= p.row_bytes; ++y; }
        }
        return;
    }
    const uint32_t units = (len - head) / 48u;
    const uint32_t tail0 = head + units * 48u;
    for (uint32_t o = tid; o < head + (len - tail0); o += kRenderBlock) {   // (< 16 + 48 bytes)
        const uint32_t b = o < head ? o : tail0 + (o - head);
        dst[b] = band_byte(p, s, b, wpx);
    }
    const uint32_t c0 = head % 3u;   // the band starts in channel 0 (row_bytes is a multiple of 3): every unit starts in channel c0
    if (c0 == 0) for (uint32_t u = tid; u < units; u += kRenderBlock) band_unit<0>(p, s, head + u * 48u, wpx, dst + head + u * 48u);
    else if (c0 == 1) for (uint32_t u = tid; u < units; u += kRenderBlock) band_unit<1>(p, s, head + u * 48u, wpx, dst + head + u * 48u);
    else for (uint32_t u = tid; u < units; u += kRenderBlock) band_unit<2>(p, s, head + u * 48u, wpx, dst + head + u * 48u);
}

}  // namespace

// rows of cells per band: about 16 KB of frame per workgroup, at most kRenderMaxBandCells cells (and `max_rows`: what the lines form
// has LDS for), and -- where the frames are few -- small enough for some thousand workgroups
static int render_band_rows(int width, int height, int gs, int n_frames, long long max_rows)
{
    const long long cell_row_bytes = (long long)gs * gs * 3 * width;
    long long rows = (16384 + cell_row_bytes - 1) / cell_row_bytes;
    rows = rows < height ? rows : height;
    const long long cap = kRenderMaxBandCells / width;   // width <= 255: >= 4
    rows = rows < cap ? rows : cap;
    rows = rows < max_rows ? rows : max_rows;
    while (rows > 1 && ((height + rows - 1) / rows) * (long long)n_frames < 1024) --rows;
    return (int)rows;
}

// The classes of a cell's pixel rows: two rows with the same answers to "in the food rows / the eye rows / the body rows / the
// border's full rows" have the same scanline in every cell.  Returns the number of classes.
static int render_row_classes(RenderParams& p)
{
    int keys[16], n = 0;
    for (int py = 0; py < p.gs; ++py) {
        const unsigned fy = (unsigned)(py - p.food_off), ey = (unsigned)(py - p.eye_y), by = (unsigned)(py - p.body_off);
        const unsigned bs = (unsigned)p.body_size, bw = (unsigned)p.border;
        const bool in_body = by < bs;
        const int key = (fy < (unsigned)p.food_size) | ((ey < (unsigned)p.eye_size) << 1) | (in_body << 2) |
                        ((in_body && (2 * bw >= bs || by < bw || by >= bs - bw)) << 3);
        int c = 0;
        while (c < n && keys[c] != key) ++c;
        if (c == n) { keys[n] = key; p.rep_py[n] = (uint8_t)py; ++n; }   // (16 keys at most)
        p.cls_of_py[py] = (uint8_t)c;
    }
    return n;
}

// Everything of the launch that follows from the shape: the form, the band height, the byte counts.  Returns the dynamic LDS size.
static size_t render_plan(RenderParams& p, int n_frames)
{
    p.row_bytes = (uint32_t)(p.W * p.gs * 3);
    p.frame_bytes = (uint32_t)(p.H * p.gs) * p.row_bytes;
    // the lines form when at least one cell row's lines fit into LDS, else the direct form
    const int n_cls = render_row_classes(p);
    p.line_stride = (p.W * p.gs + 3) / 4 * 12;
    const long long fit = (kRenderLineBytes - 16) / ((long long)n_cls * p.line_stride);
    p.n_cls = fit >= 1 ? n_cls : 0;
    p.m_gs = (1u << 20) / (uint32_t)p.gs + 1u; p.m_cls = (1u << 20) / (uint32_t)n_cls + 1u;
    p.band_rows = render_band_rows(p.W, p.H, p.gs, n_frames, fit >= 1 ? fit : (long long)p.H);
    return p.n_cls ? (size_t)p.band_rows * p.n_cls * p.line_stride + 16 : 0;
}

int rl_render_launch(rl_world* h, const rl_render_style* st, const int32_t* worlds, int n_frames, uint8_t* frames, hipStream_t stream)
{
    RenderParams p{};
    p.cell_type = h->st.cell_type; p.n_agents = h->st.n_agents; p.a_i = h->st.a_i; p.a_j = h->st.a_j; p.a_health = h->st.a_health;
    p.a_gene = h->st.a_gene; p.a_flags = h->st.a_flags;
    p.colors = st->colors; p.tiles = st->tiles; p.worlds = worlds; p.frames = frames; p.err = h->err_flag;
    p.W = h->cfg.width; p.H = h->cfg.height; p.cap = h->cfg.slot_cap; p.n_worlds = h->cfg.n_worlds; p.n_colors = st->n_colors;
    p.gs = st->grid_size; p.body_off = st->body_off; p.body_size = st->body_size; p.border = st->border;
    p.eye_size = st->eye_size; p.eye_y = st->eye_y; p.eye_x0 = st->eye_x0; p.eye_x1 = st->eye_x1;
    p.food_off = st->food_off; p.food_size = st->food_size;
    // a square that is not drawn (side <= 0) has side 0 here, and a negative border is none: the unsigned range tests then never hit
    if (p.body_size < 0) p.body_size = 0;
    if (p.eye_size < 0) p.eye_size = 0;
    if (p.food_size < 0) p.food_size = 0;
    if (p.border < 0) p.border = 0;
    const size_t dyn = render_plan(p, n_frames);
    const int bands = (p.H + p.band_rows - 1) / p.band_rows;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {   // (grid.y <= 65535)
        p.frame0 = f0;
        hipLaunchKernelGGL(k_render, dim3(bands, n_frames - f0 < 65535 ? n_frames - f0 : 65535), dim3(kRenderBlock), dyn, stream, p);
        if (hipGetLastError() != hipSuccess) { rl_set_error("rl_render: kernel launch failed"); return RL_E_LAUNCH; }
    }
    return RL_OK;
}
