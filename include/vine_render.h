/*
 * vine_render.h — C ABI of the rollout renderer (CAPTURE_VIDEO) for MI355X (gfx950).
 *
 * The reference task records 100 consecutive camera frames of env `index_to_view` every 1000 steps and saves them as a
 * video (V5:205-221, 1169-1207; V5 = isaacgymenvs/tasks/Vine5LinkMovingBase.py of the reference checkout).  Here the
 * frames are drawn by a kernel from the SoA state block of a VineHandle (include/vine.h), either on request
 * (vine_render) or as a node behind every step that decides ON THE DEVICE, from the handle's step counter, whether the
 * step just finished belongs to a capture window (vine_render_scheduled): that form can sit inside a captured hipGraph.
 *
 * Only libvine_hip.so exports this header (the CPU oracle does not: it is why these declarations are not in vine.h).
 * Errors, streams and ownership as in vine.h: 0 = ok, negative = VineStatus, message via vine_last_error(); every entry
 * point enqueues on the caller's stream and does not synchronise; the caller owns every buffer.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * THE IMAGE.  The scene is the vine's plane: world (y, z) in metres, every env in its own copy of it.  The reference's
 * camera sits at cam_target + (1, 0, 0) and looks along -x with z up (V5:206-209), so image right = +y, image up = +z.
 * The projection is orthographic: pixel (col, row) of a view, row 0 at the top, has its centre at
 *
 *     y = centre_y + (col + 0.5 - width  / 2) * metres_per_pixel
 *     z = centre_z + (height / 2 - row - 0.5) * metres_per_pixel
 *
 * evaluated in fp32.  ONE sample per pixel, at its centre; a pixel takes the material of the LAST shape in the painter's
 * order below that strictly contains its centre, else background.  A pixel is one byte: an index into the palette of
 * vine_render_palette.
 *
 * Views: view v shows env view_envs[v] and occupies the tile (v / grid_cols, v % grid_cols) of a frame of
 * (rows * height) x (grid_cols * width) pixels, rows = ceil(num_views / grid_cols), row-major, pitch grid_cols * width.
 * Tiles past num_views are background.
 *
 * Shapes, in painter's order (later ones cover earlier ones).  "px" = metres_per_pixel; a LINE of thickness t px is the
 * rectangle of half-thickness t/2 px around it; every line here has VINE_RENDER_LINE_PX = 2.5 px: whether a line's axis
 * falls on a row of pixel centres (odd height) or between two (even height), its edges stay a quarter pixel away from
 * the nearest centres, so the two or three rows it covers do not depend on rounding.
 *   1. rail               VR_RAIL      line z = 1.0 (INIT_Z), |y| <= 0.4 (LENGTH_RAIL / 2)                  V5:53, 1143
 *   2. rail soft limits   VR_LIMIT     two vertical lines at y = -+rail_soft_limit, z in [0.9, 1.1]          V5:1152-1167
 *   3. episode progress   VR_PROGRESS  line z = 1.2 from y = -0.4 to -0.4 + 0.8 * progress / max_episode_length;
 *                                      only when `progress` is given and the fraction is > 0             V5:1137-1150
 *   4. shelf boards       VR_SHELF     CREATE_SHELF: the two boards the contact code collides with, axis-aligned boxes
 *                                      (centre, half-extent) relative to (VF_SHELF_Y, VF_SHELF_Z):
 *                                      (-0.001, 0) +- (0.1995, 0.005) and (0, 0.2) +- (0.2, 0.005)
 *   5. shelf strip        VR_STRIP     CREATE_SHELF: the 2 mm front-edge strip of `shelf_link`, (0.199, 0) +- (0.001, 0.005)
 *   6. pipe walls         VR_PIPE      CREATE_PIPE: in the pipe frame (origin (VF_PIPE_Y, VF_PIPE_Z), first axis
 *                                      (cos a, sin a), second axis (-sin a, cos a), a = VF_OBJ_ANGLE + pi/2) the boxes
 *                                      [0, 0.00525] x [0, 0.34125] and [0.15015, 0.1554] x [0, 0.34125]
 *   7. target             VR_TARGET    disc of radius success_dist around (VF_TARGET_Y, VF_TARGET_Z)      V5:1124-1135
 *   8. cart               VR_CART      box (q0, 0.975) +- (0.05, 0.01)                                    URDF cart box
 *   9. links 0..4         VR_LINK_A (links 0, 2, 4) / VR_LINK_B (links 1, 3): the rectangles of the contact code.  Joint 0 at
 *                                      (q0, joint1_z); link k has world angle phi_k = phi0 + th_k, th_k = q1 + .. + q(k+1), axis
 *                                      d_k = (-sin phi_k, cos phi_k), lateral l_k = (cos phi_k, sin phi_k); joint k+1 =
 *                                      joint k + link_length * d_k; the rectangle is joint k + a * d_k + b * l_k with
 *                                      b in [-0.0381, 0.0719] and a in [0, link_length] (link 0: [-0.00575, 0.09425])
 *  10. tip marker         VR_TIP       disc of radius VINE_RENDER_TIP_RADIUS = 0.012 m around joint 5 (the `tip` body)
 * The joint angles are VF_Q0 .. VF_Q0 + 5 of the state block (q0 = cart y); forward kinematics runs in fp32 in the
 * order written above (the angle sum th_k first, one sincosf of it per link, then the rotation by phi0 with
 * (sin, cos)(phi0) rounded from double, as the step kernels form the world angles).
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_RENDER_H
#define VINE_RENDER_H

#include <stdint.h>

#include "vine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_RENDER_ABI_VERSION 1
#define VINE_RENDER_LINE_PX 2.5f       /* thickness of every line, in pixels */
#define VINE_RENDER_TIP_RADIUS 0.012f  /* metres */
#define VINE_RENDER_MAX_VIEWS 64

/* Palette indices = pixel values. */
typedef enum VineRenderMaterial {
    VR_BACKGROUND = 0,
    VR_RAIL = 1,
    VR_LIMIT = 2,
    VR_PROGRESS = 3,
    VR_CART = 4,
    VR_LINK_A = 5,
    VR_LINK_B = 6,
    VR_TIP = 7,
    VR_TARGET = 8,
    VR_SHELF = 9,
    VR_STRIP = 10,
    VR_PIPE = 11,
    VR_NUM_MATERIALS = 12
} VineRenderMaterial;

typedef struct VineRenderConfig {
    int32_t abi_version;       /* must be VINE_RENDER_ABI_VERSION */
    int32_t width, height;     /* of one view; default 400 x 225: the reference's camera, a quarter of Isaac Gym's default
                                  1600 x 900 (V5:213-215) */
    int32_t num_views;         /* 1 .. VINE_RENDER_MAX_VIEWS; default 1 */
    int32_t grid_cols;         /* views per frame row; default 1 */
    int32_t num_frames;        /* frames per capture window, = slots of the ring; default 100 (V5:218) */
    int32_t capture_every;     /* a window opens at every multiple of this many steps; default 1000 (V5:219) */
    float centre_y, centre_z;  /* world point at the centre of every view; default (0, 1.0): cam_target of V5:207 with the
                                  tip over the origin */
    float metres_per_pixel;    /* default 2.0 / 400: the width a 90 degree horizontal field of view covers at the
                                  camera's distance of 1 m (V5:208).  The 90 degrees are Isaac Gym's CameraProperties default
                                  AS RECALLED; nothing in the reference tree pins the value. */
} VineRenderConfig;

int vine_render_config_default(VineRenderConfig* cfg);
int vine_render_config_size(void);        /* sizeof(VineRenderConfig): checked by the ctypes mirror */

/* Bytes of one frame ((rows * height) * (grid_cols * width)) and of the ring (num_frames frames); negative = VineStatus. */
int64_t vine_render_frame_bytes(const VineRenderConfig* cfg);
int64_t vine_render_ring_bytes(const VineRenderConfig* cfg);

/* The fixed palette: rgb[VR_NUM_MATERIALS][3]; *n (optional) receives VR_NUM_MATERIALS. */
int vine_render_palette(uint8_t rgb[][3], int* n);

/* Draw the CURRENT state once.
 * view_envs  device int32[num_views], each in [0, num_envs): checked on the device -- a view whose env is out of range is
 *            drawn as background (nothing is read out of bounds)
 * progress   device int64[num_envs] (the step's progress_buf) or NULL: no progress bar
 * out        device uint8, vine_render_frame_bytes(cfg) bytes */
int vine_render(VineHandle* h, const VineRenderConfig* cfg, const int32_t* view_envs, const int64_t* progress,
                uint8_t* out, void* stream);

/* The graph node.  Enqueued behind a step launch on the same stream, it reads the handle's device step counter
 * c = steps completed; the step just finished has index s = c - 1 and is drawn into slot s % capture_every of `ring` iff
 * that is < num_frames: the reference starts a window when num_steps % capture_video_every == 0 and increments num_steps
 * after the check (V5:1170-1173, 1207).  Otherwise (and when c == 0) every workgroup returns at once.  Nothing that
 * changes from step to step is a kernel argument, so a captured launch replays correctly.
 * ring       device uint8, vine_render_ring_bytes(cfg) bytes: [num_frames][rows * height][grid_cols * width] */
int vine_render_scheduled(VineHandle* h, const VineRenderConfig* cfg, const int32_t* view_envs, const int64_t* progress,
                          uint8_t* ring, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_RENDER_H */
