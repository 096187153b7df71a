// vine_render.hip — the rollout renderer (CAPTURE_VIDEO) for MI355X (gfx950): include/vine_render.h.
//
// One launch draws every view of a frame.  A workgroup of 256 lanes owns a tile of 64 x 16 pixels of one view, every lane
// four neighbouring pixels of a row (one 4-byte store).  Per workgroup: lanes 0..4 take sin / cos of the five link
// angles, lane 0 then builds the view's shapes (at most 17 oriented boxes and discs) and keeps in LDS only those whose
// bounding box meets the tile; every pixel tests that short list in painter's order.  A tile no shape reaches writes
// background without testing anything.
//
// The scheduled form reads the step counter of the handle (vine_observer.h vine_steps_completed: two 8-byte loads, uniform, so they are
// scalar loads) and returns at once outside a capture window: no LDS, no barrier, no store on that path.
// The shapes are those of the contact code (vine_geometry.h).  Plain C++ stores only.

#include <hip/hip_runtime.h>

#include "../../include/vine_render.h"
#include "vine_geometry.h"
#include "vine_observer.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 16, THREADS = 256, PX = 4;    // THREADS * PX == TILE_W * TILE_H
constexpr int MAX_PRIMS = 20;

struct RenderParams {
    int W, H, views, cols, cells, tiles_x, pitch, num_frames, capture_every;
    int n, glog, max_len;
    unsigned flags;
    float cy, cz, mpp;
    float L, z1, s0, c0, soft_limit, success_dist;
    long long frame_bytes;
};

// An oriented box: centre (cy, cz), unit axis (uy, uz), half-extents hu along the axis and hv across it; a disc has
// hv < 0 and its radius in hu.
struct Prim {
    float cy, cz, uy, uz, hu, hv;
    int mat;
};

struct PrimList {
    int count;
    Prim p[MAX_PRIMS];
};

// Appends the shape if its bounding box meets the tile's box of pixel centres [ty0, ty1] x [tz0, tz1].
__device__ __forceinline__ void push(PrimList& l, float ty0, float ty1, float tz0, float tz1, float cy, float cz, float uy,
                                     float uz, float hu, float hv, int mat) {
    float ey, ez;
    if (hv < 0.0f) {
        ey = hu; ez = hu;
    } else {
        ey = fabsf(uy) * hu + fabsf(uz) * hv;
        ez = fabsf(uz) * hu + fabsf(uy) * hv;
    }
    if (cy + ey < ty0 || cy - ey > ty1 || cz + ez < tz0 || cz - ez > tz1) return;
    if (l.count >= MAX_PRIMS) return;
    l.p[l.count++] = Prim{cy, cz, uy, uz, hu, hv, mat};
}
__device__ __forceinline__ void push_box(PrimList& l, float ty0, float ty1, float tz0, float tz1, float cy, float cz, float hy,
                                         float hz, int mat) {
    push(l, ty0, ty1, tz0, tz1, cy, cz, 1.0f, 0.0f, hy, hz, mat);
}

template <bool SCHEDULED>
__global__ __launch_bounds__(THREADS) void vine_render_kernel(const RenderParams R, const float* __restrict__ st,
                                                              const int* __restrict__ view_envs,
                                                              const long long* __restrict__ progress,
                                                              const unsigned long long* __restrict__ counters,
                                                              unsigned char* __restrict__ out) {
    if (SCHEDULED) {
        const unsigned long long c = vine_steps_completed(counters, R.glog);
        if (c == 0ull) return;
        const unsigned long long slot = (c - 1ull) % (unsigned long long)R.capture_every;
        if (slot >= (unsigned long long)R.num_frames) return;
        out += (long long)slot * R.frame_bytes;
    }
    __shared__ PrimList list;
    __shared__ float sn[VINE_NUM_LINKS], cs[VINE_NUM_LINKS];

    const int cell = blockIdx.y;                         // tile of the frame's grid of views
    const int tx = blockIdx.x % R.tiles_x, tyi = blockIdx.x / R.tiles_x;
    const int col0 = tx * TILE_W, row0 = tyi * TILE_H;
    int env = -1;
    if (cell < R.views) {
        env = view_envs[cell];
        if (env < 0 || env >= R.n) env = -1;
    }
    const float halfw = 0.5f * (float)R.W, halfh = 0.5f * (float)R.H;
    if (env >= 0) {
        const int n = R.n;
        if (threadIdx.x < VINE_NUM_LINKS) {
            float th = 0.0f;
            for (int i = 0; i <= (int)threadIdx.x; ++i) th += st[(VF_Q0 + 1 + i) * n + env];
            float s, c;
            sincosf(th, &s, &c);
            sn[threadIdx.x] = R.s0 * c + R.c0 * s;       // world angle phi0 + th, as the step kernels form it
            cs[threadIdx.x] = R.c0 * c - R.s0 * s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            list.count = 0;
            const int colN = min(col0 + TILE_W, R.W) - 1, rowN = min(row0 + TILE_H, R.H) - 1;
            const float m = R.mpp, eps = 0.5f * m;       // half a pixel of slack: culling must never drop a shape a pixel hits
            const float ty0 = R.cy + ((float)col0 + 0.5f - halfw) * m - eps, ty1 = R.cy + ((float)colN + 0.5f - halfw) * m + eps;
            const float tz1 = R.cz + (halfh - (float)row0 - 0.5f) * m + eps, tz0 = R.cz + (halfh - (float)rowN - 0.5f) * m - eps;
            const float lh = 0.5f * VINE_RENDER_LINE_PX * m;
            push_box(list, ty0, ty1, tz0, tz1, 0.0f, SCENE_INIT_Z, SCENE_RAIL_HALF, lh, VR_RAIL);
            push_box(list, ty0, ty1, tz0, tz1, -R.soft_limit, SCENE_INIT_Z, lh, 0.1f, VR_LIMIT);
            push_box(list, ty0, ty1, tz0, tz1, R.soft_limit, SCENE_INIT_Z, lh, 0.1f, VR_LIMIT);
            if (progress) {
                const float frac = (float)progress[env] / (float)R.max_len;
                if (frac > 0.0f) {
                    const float half = SCENE_RAIL_HALF * frac;            // the bar spans [-0.4, -0.4 + 0.8 frac]
                    push_box(list, ty0, ty1, tz0, tz1, -SCENE_RAIL_HALF + half, SCENE_INIT_Z + 0.2f, half, lh, VR_PROGRESS);
                }
            }
            if (R.flags & VINE_FLAG_CREATE_SHELF) {
                const float board[2][4] = SHELF_BOARDS;
                const float strip[4] = SHELF_STRIP;
                const float sy = st[VF_SHELF_Y * n + env], sz = st[VF_SHELF_Z * n + env];
                for (int b = 0; b < 2; ++b)
                    push_box(list, ty0, ty1, tz0, tz1, sy + board[b][0], sz + board[b][1], board[b][2], board[b][3], VR_SHELF);
                push_box(list, ty0, ty1, tz0, tz1, sy + strip[0], sz + strip[1], strip[2], strip[3], VR_STRIP);
            }
            if (R.flags & VINE_FLAG_CREATE_PIPE) {
                float pst, pct;
                sincosf(st[VF_OBJ_ANGLE * n + env] + 1.5707963267948966f, &pst, &pct);
                const PipePose T = pipe_pose(st[VF_PIPE_Y * n + env], st[VF_PIPE_Z * n + env], pct, pst);
                for (int w = 0; w < 2; ++w) {
                    const float a = (w ? PIPE_OUTER - PIPE_WALL : 0.0f) + 0.5f * PIPE_WALL, b = 0.5f * PIPE_LEN;
                    push(list, ty0, ty1, tz0, tz1, T.y + a * T.ct - b * T.st, T.z + a * T.st + b * T.ct, -T.st, T.ct,
                         0.5f * PIPE_LEN, 0.5f * PIPE_WALL, VR_PIPE);
                }
            }
            push(list, ty0, ty1, tz0, tz1, st[VF_TARGET_Y * n + env], st[VF_TARGET_Z * n + env], 1.0f, 0.0f, R.success_dist,
                 -1.0f, VR_TARGET);
            float py = st[VF_Q0 * n + env], pz = R.z1;
            push_box(list, ty0, ty1, tz0, tz1, py, SCENE_CART_Z, SCENE_CART_HY, SCENE_CART_HZ, VR_CART);
            for (int k = 0; k < VINE_NUM_LINKS; ++k) {
                const float dy = -sn[k], dz = cs[k], ly = cs[k], lz = sn[k];
                const float z0 = (k == 0) ? LINK0_Z0 : 0.0f, z1 = (k == 0) ? LINK0_Z1 : R.L;
                const float a = 0.5f * (z0 + z1), b = 0.5f * (LINK_Y0 + LINK_Y1);
                push(list, ty0, ty1, tz0, tz1, py + a * dy + b * ly, pz + a * dz + b * lz, dy, dz, 0.5f * (z1 - z0),
                     0.5f * (LINK_Y1 - LINK_Y0), (k & 1) ? VR_LINK_B : VR_LINK_A);
                py += R.L * dy; pz += R.L * dz;
            }
            push(list, ty0, ty1, tz0, tz1, py, pz, 1.0f, 0.0f, VINE_RENDER_TIP_RADIUS, -1.0f, VR_TIP);
        }
        __syncthreads();
    }

    const int lx = (threadIdx.x & (TILE_W / PX - 1)) * PX, lyr = threadIdx.x / (TILE_W / PX);
    const int col = col0 + lx, row = row0 + lyr;
    if (row >= R.H || col >= R.W) return;
    unsigned mat[PX] = {VR_BACKGROUND, VR_BACKGROUND, VR_BACKGROUND, VR_BACKGROUND};
    const int count = (env >= 0) ? list.count : 0;
    if (count > 0) {
        const float z = R.cz + (halfh - (float)row - 0.5f) * R.mpp;
        float y[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) y[j] = R.cy + ((float)(col + j) + 0.5f - halfw) * R.mpp;
        for (int i = 0; i < count; ++i) {
            const Prim p = list.p[i];
            const float ez = z - p.cz;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float ey = y[j] - p.cy;
                bool hit;
                if (p.hv < 0.0f) {
                    hit = ey * ey + ez * ez < p.hu * p.hu;
                } else {
                    const float a = ey * p.uy + ez * p.uz, b = ez * p.uy - ey * p.uz;
                    hit = fabsf(a) < p.hu && fabsf(b) < p.hv;
                }
                if (hit) mat[j] = (unsigned)p.mat;
            }
        }
    }
    const int cr = cell / R.cols, cc = cell % R.cols;
    unsigned char* dst = out + ((long long)cr * R.H + row) * R.pitch + (long long)cc * R.W + col;
    if (col + PX <= R.W && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
        *reinterpret_cast<unsigned*>(dst) = mat[0] | (mat[1] << 8) | (mat[2] << 16) | (mat[3] << 24);
    } else {
        // the tail of a width that is not a multiple of four, and rows whose start is not 4-byte aligned
#pragma unroll
        for (int j = 0; j < PX; ++j)
            if (col + j < R.W) dst[j] = (unsigned char)mat[j];
    }
}

int validate(const VineRenderConfig* c) {
    if (!c) return vine_invalid_arg("render config is NULL");
    if (c->abi_version != VINE_RENDER_ABI_VERSION) return vine_invalid_arg("VineRenderConfig.abi_version mismatch");
    if (c->width < 1 || c->width > 8192 || c->height < 1 || c->height > 8192) return vine_invalid_arg("render width / height out of range");
    if (c->num_views < 1 || c->num_views > VINE_RENDER_MAX_VIEWS) return vine_invalid_arg("num_views out of range");
    if (c->grid_cols < 1 || c->grid_cols > c->num_views) return vine_invalid_arg("grid_cols out of range");
    if (c->num_frames < 1 || c->capture_every < c->num_frames) return vine_invalid_arg("need 1 <= num_frames <= capture_every");
    if (!(c->metres_per_pixel > 0.0f)) return vine_invalid_arg("metres_per_pixel must be positive");
    return VINE_OK;
}

int grid_rows(const VineRenderConfig* c) { return (c->num_views + c->grid_cols - 1) / c->grid_cols; }

int launch(VineHandle* h, const VineRenderConfig* cfg, const int32_t* view_envs, const int64_t* progress, uint8_t* out,
           void* stream, bool scheduled) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!h || !view_envs || !out) return vine_invalid_arg("null argument to vine_render");
    VineHandleInfo info;
    rc = vine_handle_info(h, &info);
    if (rc) return rc;
    RenderParams R;
    R.W = cfg->width; R.H = cfg->height; R.views = cfg->num_views; R.cols = cfg->grid_cols;
    R.cells = grid_rows(cfg) * cfg->grid_cols;
    R.tiles_x = (R.W + TILE_W - 1) / TILE_W;
    R.pitch = R.cols * R.W;
    R.num_frames = cfg->num_frames; R.capture_every = cfg->capture_every;
    R.n = info.n; R.glog = info.glog; R.max_len = info.max_len; R.flags = info.flags;
    R.cy = cfg->centre_y; R.cz = cfg->centre_z; R.mpp = cfg->metres_per_pixel;
    R.L = info.L; R.z1 = info.z1; R.s0 = info.s0; R.c0 = info.c0;
    R.soft_limit = info.soft_limit; R.success_dist = info.success_dist;
    R.frame_bytes = vine_render_frame_bytes(cfg);
    const int tiles_y = (R.H + TILE_H - 1) / TILE_H;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    const dim3 grid(R.tiles_x * tiles_y, R.cells), block(THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (scheduled)
        hipLaunchKernelGGL(vine_render_kernel<true>, grid, block, 0, s, R, info.state, (const int*)view_envs,
                           (const long long*)progress, info.counters, out);
    else
        hipLaunchKernelGGL(vine_render_kernel<false>, grid, block, 0, s, R, info.state, (const int*)view_envs,
                           (const long long*)progress, info.counters, out);
    return vine_launch_status("vine_render");
}

const uint8_t PALETTE[VR_NUM_MATERIALS][3] = {
    {245, 245, 245},   // VR_BACKGROUND
    {90, 90, 90},      // VR_RAIL
    {230, 26, 26},     // VR_LIMIT     (0.9, 0.1, 0.1), V5:1164
    {26, 230, 26},     // VR_PROGRESS  (0.1, 0.9, 0.1), V5:1149
    {40, 40, 40},      // VR_CART
    {30, 100, 200},    // VR_LINK_A
    {110, 170, 240},   // VR_LINK_B
    {250, 160, 0},     // VR_TIP
    {0, 200, 0},       // VR_TARGET    (0, 1, 0), V5:1127, darkened against the light background
    {150, 100, 50},    // VR_SHELF
    {90, 50, 20},      // VR_STRIP
    {130, 130, 150},   // VR_PIPE
};

}  // namespace

extern "C" {

int vine_render_config_default(VineRenderConfig* c) {
    if (!c) return vine_invalid_arg("render config is NULL");
    c->abi_version = VINE_RENDER_ABI_VERSION;
    c->width = 400; c->height = 225;
    c->num_views = 1; c->grid_cols = 1;
    c->num_frames = 100; c->capture_every = 1000;
    c->centre_y = 0.0f; c->centre_z = SCENE_INIT_Z;
    c->metres_per_pixel = 2.0f / 400.0f;
    return VINE_OK;
}

int vine_render_config_size(void) { return (int)sizeof(VineRenderConfig); }

int64_t vine_render_frame_bytes(const VineRenderConfig* c) {
    const int rc = validate(c);
    if (rc) return rc;
    return (int64_t)grid_rows(c) * c->height * c->grid_cols * c->width;
}

int64_t vine_render_ring_bytes(const VineRenderConfig* c) {
    const int64_t f = vine_render_frame_bytes(c);
    return f < 0 ? f : f * c->num_frames;
}

int vine_render_palette(uint8_t rgb[][3], int* n) {
    if (!rgb) return vine_invalid_arg("palette buffer is NULL");
    for (int i = 0; i < VR_NUM_MATERIALS; ++i)
        for (int k = 0; k < 3; ++k) rgb[i][k] = PALETTE[i][k];
    if (n) *n = VR_NUM_MATERIALS;
    return VINE_OK;
}

int vine_render(VineHandle* h, const VineRenderConfig* cfg, const int32_t* view_envs, const int64_t* progress, uint8_t* out,
                void* stream) {
    return launch(h, cfg, view_envs, progress, out, stream, false);
}

int vine_render_scheduled(VineHandle* h, const VineRenderConfig* cfg, const int32_t* view_envs, const int64_t* progress,
                          uint8_t* ring, void* stream) {
    return launch(h, cfg, view_envs, progress, ring, stream, true);
}

}  // extern "C"
