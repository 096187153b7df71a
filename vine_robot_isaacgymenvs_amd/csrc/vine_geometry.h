// vine_geometry.h — the planar shapes of the scene, shared by the contact code of the step kernels (vine_hip.hip) and by
// the renderer (vine_render.hip), so that a video shows exactly what the contact code collides with.  Constants and one
// inlined helper only: including it changes no instruction of the step kernels.
#ifndef VINE_GEOMETRY_H
#define VINE_GEOMETRY_H

#include <hip/hip_runtime.h>

// Link rectangle in link-local coordinates: lateral y in [LINK_Y0, LINK_Y1] (main cylinder r = 0.0381 + FPAM cylinder at
// y = 0.055, r = 0.0169), axial z in [0, link_length]; link_0 (length 0.1 centred at 0.04425) in [LINK0_Z0, LINK0_Z1].
#define LINK_Y0 (-0.0381f)
#define LINK_Y1 0.0719f
#define LINK0_Z0 -0.00575f
#define LINK0_Z1 0.09425f
// The two boards of the shelf, (cy, cz, hy, hz) relative to the shelf's root, and the front-edge strip of `shelf_link`
// (its two front corners at y = +0.2, z = -+0.005 are what the contact code tests against the links).
#define SHELF_BOARDS {{-0.001f, 0.0f, 0.1995f, 0.005f}, {0.0f, 0.2f, 0.2f, 0.005f}}
#define SHELF_STRIP {0.199f, 0.0f, 0.001f, 0.005f}
// The pipe's cross-section in the pipe frame: two walls of thickness PIPE_WALL, outer faces PIPE_OUTER apart, PIPE_LEN long.
#define PIPE_LEN 0.34125f
#define PIPE_WALL 0.00525f
#define PIPE_OUTER 0.1554f
struct PipePose { float y, z, ct, st, ccy, ccz; };      // origin, cos / sin of the tube's axis angle, centre of its box
__device__ __forceinline__ PipePose pipe_pose(float pipe_y, float pipe_z, float ct, float st) {
    const float hcy = 0.5f * PIPE_OUTER, hcz = 0.5f * PIPE_LEN;
    return PipePose{pipe_y, pipe_z, ct, st, pipe_y + hcy * ct - hcz * st, pipe_z + hcy * st + hcz * ct};
}
// Scene constants of the reference task (V5:48-53, 85; URDF cart box 0.07 x 0.1 x 0.02 at z = 0.975).
#define SCENE_INIT_Z 1.0f
#define SCENE_RAIL_HALF 0.4f
#define SCENE_CART_Z 0.975f
#define SCENE_CART_HY 0.05f
#define SCENE_CART_HZ 0.01f

#endif
