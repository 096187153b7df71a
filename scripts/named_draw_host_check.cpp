// named_draw_host_check.cpp — the shared check of one named draw (csrc/vine_named_draw.h, named_check) through two of the
// spec entry points that use it, vine_env_push_spec and vine_env_sensor_spec, as a stand-alone program for a sanitizer build
// of the HOST code (no device is touched, neither entry point needs a handle):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/named_draw_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_env_push.hip \
//         vine_robot_isaacgymenvs_amd/csrc/vine_env_sensor.hip -o build/named_draw_host_check
//   ./build/named_draw_host_check
//
// What the two units need of vine_hip.hip is stood in for here, as scripts/env_target_host_check.cpp does.  Exit status 0 and
// "named draw host check ok" when each of the eight shared refusals -- reserved, a number that is not finite, a range
// without finite lo <= hi, the extent of a value list, its radix, a listed value that is not finite, an absent name, an
// unknown form -- comes out of either unit under that unit's prefix and the name's, a value's own refusal behind the
// finiteness of that value, and a good spec passes.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../include/vine_env_push.h"
#include "../include/vine_env_sensor.h"
#include "../vine_robot_isaacgymenvs_amd/csrc/vine_observer.h"

static char g_err[256];
extern "C" {
void vine_set_error(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
int vine_handle_info(VineHandle*, VineHandleInfo*) { return VINE_ERR_INVALID_ARG; }
int vine_env_tables_of(VineHandle*, const float**, const float**, unsigned*) { return VINE_ERR_INVALID_ARG; }
int vine_num_obs(const VineConfig*) { return 28; }
int vine_env_inertia_row(const VineConfig*, float row[VI_COUNT]) {
    for (int r = 0; r < VI_COUNT; ++r) row[r] = 1.0f + (float)r;
    return VINE_OK;
}
}

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_err);
    }
}

static VineEnvRedrawName number(double v) {
    VineEnvRedrawName nm;
    memset(&nm, 0, sizeof nm);
    nm.form = VINE_REDRAW_NUMBER;
    nm.lo = nm.hi = v;
    nm.radix = 1;
    return nm;
}
static VineEnvRedrawName range(double lo, double hi) {
    VineEnvRedrawName nm = number(lo);
    nm.form = VINE_REDRAW_RANGE;
    nm.hi = hi;
    return nm;
}
static VineEnvRedrawName list(int first, int count) {
    VineEnvRedrawName nm = number(0.0);
    nm.form = VINE_REDRAW_VALUES;
    nm.values_first = first;
    nm.values_count = count;
    return nm;
}

// [0, 1]: good for every name; [2]: not finite; [3]: finite, and negative -- no name may take it
static const double kValues[4] = {0.0, 0.5, NAN, -1.0};

static VineConfig config() {
    VineConfig c;
    memset(&c, 0, sizeof c);
    c.abi_version = VINE_ABI_VERSION;
    c.num_envs = 4;
    c.clip_observations = 5.0f;
    c.seed = 11;
    return c;
}

// slot 1 of both units (PUSH_IMPULSE, SENSOR_HOLD) carries the change; slot 0 stays good
static int push(const VineEnvRedrawName& second, VineEnvPushSpec* out) {
    const VineConfig c = config();
    const VineEnvRedrawName names[VPU_NAMES] = {number(0.1), second};
    const int32_t points[1] = {5};
    g_err[0] = 0;
    return vine_env_push_spec(&c, names, kValues, kValues, 4, points, 1, 0, out);
}
static int sensor(const VineEnvRedrawName& second, VineEnvSensorSpec* out) {
    const VineConfig c = config();
    const VineEnvRedrawName names[VSN_NAMES] = {number(1.0), second, number(0.0)};
    g_err[0] = 0;
    return vine_env_sensor_spec(&c, names, kValues, kValues, 4, 0xFFu, 0, out);
}

static void refused(const char* why, VineEnvRedrawName nm) {
    char want[200];
    VineEnvPushSpec P;
    VineEnvSensorSpec S;
    snprintf(want, sizeof want, "env push spec: PUSH_IMPULSE: %s", why);
    expect(push(nm, &P) == VINE_ERR_INVALID_ARG && strstr(g_err, want), want);
    snprintf(want, sizeof want, "env sensor spec: SENSOR_HOLD: %s", why);
    expect(sensor(nm, &S) == VINE_ERR_INVALID_ARG && strstr(g_err, want), want);
}

int main() {
    VineEnvPushSpec P;
    VineEnvSensorSpec S;
    expect(push(number(0.5), &P) == VINE_OK && P.checked == 1u && P.name[VPU_IMPULSE].form == VINE_REDRAW_NUMBER, "a good push spec");
    expect(sensor(range(0.0, 0.5), &S) == VINE_OK && S.checked == 1u && S.name[VSN_HOLD].hi == 0.5, "a good sensor spec");
    expect(push(list(0, 2), &P) == VINE_OK && P.name[VPU_IMPULSE].values_count == 2, "a push spec with a value list");
    expect(sensor(list(0, 2), &S) == VINE_OK, "a sensor spec with a value list");

    // the eight, in the order the shared check makes them
    VineEnvRedrawName nm = number(0.5);
    nm.reserved = 1;
    refused("reserved must be 0", nm);
    refused("the number is not finite", number(INFINITY));
    refused("a range needs finite lo <= hi", range(0.5, 0.25));
    refused("a range needs finite lo <= hi", range(0.0, NAN));
    refused("the extent of the value list lies outside the values array", list(3, 2));
    refused("the extent of the value list lies outside the values array", list(-1, 2));
    refused("the extent of the value list lies outside the values array", list(0, 0));
    nm = list(0, 2);
    nm.radix = 0;
    refused("radix must be at least 1", nm);
    refused("a listed value is not finite", list(1, 2));
    nm = number(0.0);
    nm.form = VINE_REDRAW_ABSENT;
    refused("absent: every name needs a number, a range or a value list", nm);
    nm.form = 9;
    refused("unknown form", nm);

    // a spec wrong in two ways names the earlier of the two: reserved before the form, the extent before the radix, a value
    // that is not finite before a later one the unit refuses, finiteness of a number before the unit's word on it
    nm = number(NAN);
    nm.reserved = 2;
    refused("reserved must be 0", nm);
    nm = list(3, 2);
    nm.radix = 0;
    refused("the extent of the value list lies outside the values array", nm);
    refused("a listed value is not finite", list(2, 2));
    refused("the number is not finite", number(-INFINITY));

    // the unit's own word on a single value, through the shared walk: a number, either end of a range, a listed value
    expect(push(number(-1.0), &P) == VINE_ERR_INVALID_ARG && strstr(g_err, "env push spec: PUSH_IMPULSE: must not be negative"), "impulse, a number");
    expect(sensor(number(-1.0), &S) == VINE_ERR_INVALID_ARG && strstr(g_err, "env sensor spec: SENSOR_HOLD: must lie in [0, 1)"), "hold, a number");
    expect(sensor(range(0.0, 1.0), &S) == VINE_ERR_INVALID_ARG && strstr(g_err, "SENSOR_HOLD: must lie in [0, 1)"), "hold, the upper end");
    expect(sensor(list(3, 1), &S) == VINE_ERR_INVALID_ARG && strstr(g_err, "SENSOR_HOLD: must lie in [0, 1)"), "hold, a listed value");
    expect(push(range(-1.0, 0.5), &P) == VINE_ERR_INVALID_ARG && strstr(g_err, "PUSH_IMPULSE: must not be negative"), "impulse, the lower end");
    expect(push(list(3, 1), &P) == VINE_ERR_INVALID_ARG && strstr(g_err, "PUSH_IMPULSE: must not be negative"), "impulse, a listed value");
    // the units' own checks over the envelope
    expect(push(number(0.0), &P) == VINE_ERR_INVALID_ARG && strstr(g_err, "PUSH_IMPULSE: constant zero: nothing to do"), "constant zero");
    expect(push(list(0, 1), &P) == VINE_ERR_INVALID_ARG && strstr(g_err, "PUSH_IMPULSE: constant zero: nothing to do"), "a list of zeros");
    {
        const VineConfig c = config();
        const VineEnvRedrawName zeros[VSN_NAMES] = {number(0.0), list(0, 1), range(0.0, 0.0)};
        g_err[0] = 0;
        expect(vine_env_sensor_spec(&c, zeros, kValues, kValues, 4, 0xFFu, 0, &S) == VINE_ERR_INVALID_ARG &&
                   strstr(g_err, "are all constant zero: nothing to do"), "all constant zero");
        expect(vine_env_sensor_spec(&c, zeros, kValues, kValues, 4, 0xFFu, 1, &S) == VINE_OK, "all zero, per episode");
    }

    if (failures) return 1;
    printf("named draw host check ok\n");
    return 0;
}
