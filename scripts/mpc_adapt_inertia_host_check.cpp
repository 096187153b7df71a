// mpc_adapt_inertia_host_check.cpp — the host-side entry points of csrc/vine_mpc_adapt_inertia.hip on their refusal paths, as a
// stand-alone program for a sanitizer build of the HOST code (no device is touched: every call below returns before its launch):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=fast-honor-pragmas \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip scripts/mpc_adapt_inertia_host_check.cpp vine_robot_isaacgymenvs_amd/csrc/vine_mpc_adapt_inertia.hip \
//         -o build/mpc_adapt_inertia_host_check
//   ./build/mpc_adapt_inertia_host_check
//
// The functions the unit needs of vine_hip.hip (vine_observer.h) are stood in for here, so that the unit is checked alone: the
// stand-in handle has `g_envs` envs and the tables `g_params` / `g_inertia` bound, and with g_envs < 0 it is refused outright.
// Exit status 0 and "mpc adapt inertia host check ok" when every refusal is what include/vine_mpc_adapt_inertia.h says.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/vine_mpc_adapt_inertia.h"
#include "../vine_robot_isaacgymenvs_amd/csrc/vine_observer.h"

static char g_err[256];
static int g_envs = -1;
static const float* g_params = nullptr;
static const float* g_inertia = nullptr;
extern "C" {
void vine_set_error(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
int vine_handle_info(VineHandle*, VineHandleInfo* out) {
    if (g_envs < 0) {
        vine_set_error("stand-in handle");
        return VINE_ERR_INVALID_ARG;
    }
    memset(out, 0, sizeof *out);
    out->n = g_envs;
    out->env_params = g_params;
    return VINE_OK;
}
const float* vine_reward_matrix_of(VineHandle*) { return nullptr; }
int vine_env_tables_of(VineHandle*, const float** params, const float** inertia, unsigned* env_id_offset) {
    *params = g_params;
    *inertia = g_inertia;
    *env_id_offset = 0;
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

// The base configuration of include/vine_mpc_adapt.h with three plants of 16 samples and DAMPING as its one dimension.
static VineMpcAdaptConfig base() {
    VineMpcAdaptConfig c;
    memset(&c, 0, sizeof c);
    c.abi_version = VINE_MPC_ADAPT_ABI_VERSION;
    c.num_plants = 3;
    c.samples = 16;
    c.window = 8;
    c.every = 8;
    c.num_dims = 1;
    c.min_steps = 4;
    c.temperature = 0.1;
    c.rate = 0.5;
    for (int f = 0; f < 6; ++f) c.weights[f] = 1.0f;
    c.dims[0].first_row = VP_DAMPING;
    c.dims[0].num_rows = 1;
    c.dims[0].lo = 0.005;
    c.dims[0].hi = 0.1;
    return c;
}

// A mass configuration with LINK_MASS over [0.7, 1.4] on plausible masses.
static VineMpcAdaptInertiaConfig masses() {
    VineMpcAdaptInertiaConfig m;
    vine_mpc_adapt_inertia_config_default(&m);
    m.num_mass_dims = 1;
    m.dims[0].name = VINE_MPC_ADAPT_INERTIA_LINK;
    m.dims[0].lo = 0.7;
    m.dims[0].hi = 1.4;
    m.dims[0].std_floor = 0.007;
    m.base_inertia[VI_CART_MASS] = 1.0f;
    for (int i = 0; i < VINE_NUM_LINKS; ++i) {
        m.base_inertia[VI_LINK_MASS0 + i] = 0.05f;
        m.base_inertia[VI_LINK_INERTIA0 + i] = 1e-4f;
    }
    m.link_length = 0.2f;
    m.link_com = 0.1f;
    m.gravity = 9.81f;
    return m;
}

static float g_table[4];
static double g_d[4];
static int64_t g_i64[4];
static int32_t g_i32[4];
static uint8_t g_u8[4];

static int pin(VineHandle* h, const VineMpcAdaptConfig* c, const VineMpcAdaptInertiaConfig* m, float* table) {
    return vine_mpc_adapt_inertia_pin(h, c, m, table, g_d, g_d, g_i64, nullptr);
}
static int estimate(VineHandle* h, const VineMpcAdaptConfig* c, const VineMpcAdaptInertiaConfig* m, float* table) {
    return vine_mpc_adapt_inertia_estimate(h, c, m, table, g_d, g_i32, g_u8, g_d, g_d, g_d, g_d, g_i64, nullptr, nullptr);
}

template <class Change>
static void refused_everywhere(const char* word, Change change, int status = VINE_ERR_INVALID_ARG) {
    VineMpcAdaptConfig c = base();
    VineMpcAdaptInertiaConfig m = masses();
    change(c, m);
    alignas(8) static char buf[64];
    VineHandle* h = reinterpret_cast<VineHandle*>(buf);
    g_err[0] = 0;
    expect(pin(h, &c, &m, g_table) == status && strstr(g_err, word) != nullptr, word);
    g_err[0] = 0;
    expect(estimate(h, &c, &m, g_table) == status && strstr(g_err, word) != nullptr, word);
}

int main() {
    typedef VineMpcAdaptConfig B;
    typedef VineMpcAdaptInertiaConfig I;
    I m;
    memset(&m, 0xff, sizeof m);
    expect(vine_mpc_adapt_inertia_config_default(nullptr) == VINE_ERR_INVALID_ARG, "default(NULL)");
    expect(vine_mpc_adapt_inertia_config_default(&m) == VINE_OK, "default");
    expect(m.abi_version == VINE_MPC_ADAPT_INERTIA_ABI_VERSION && m.num_mass_dims == 0 && m.dims[2].hi == 0.0 &&
               m.base_inertia[10] == 0.0f && m.link_length == 0.0f && m.gravity == 0.0f, "default values");
    expect(vine_mpc_adapt_inertia_config_size() == (int)sizeof(I) && sizeof(I) == 160, "size");

    const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    g_envs = -1;      // the handle is refused outright: everything below must be refused in front of it
    // what vine_mpc_adapt.hip refuses of the base configuration, in its words
    refused_everywhere("VineMpcAdaptConfig.abi_version", [](B& c, I&) { c.abi_version = 7; });
    refused_everywhere("num_plants", [](B& c, I&) { c.num_plants = 0; });
    refused_everywhere("samples", [](B& c, I&) { c.samples = 1; });
    refused_everywhere("window", [](B& c, I&) { c.window = 33; c.every = 33; });
    refused_everywhere("window <= every", [](B& c, I&) { c.every = 4; });
    refused_everywhere("num_dims", [](B& c, I&) { c.num_dims = 0; });
    refused_everywhere("min_steps", [](B& c, I&) { c.min_steps = 9; });
    refused_everywhere("forget_on_reset", [](B& c, I&) { c.forget_on_reset = 2; });
    refused_everywhere("temperature", [](B& c, I&) { c.temperature = 0.0; });
    refused_everywhere("rate", [=](B& c, I&) { c.rate = nan; });
    refused_everywhere("weights", [](B& c, I&) { c.weights[3] = -1.0f; });
    refused_everywhere("base_rows", [=](B& c, I&) { c.base_rows[2] = finf; });
    refused_everywhere("ACTION_DELAY", [](B& c, I&) { c.dims[0].first_row = VP_ACTION_DELAY; }, VINE_ERR_UNSUPPORTED);
    refused_everywhere("neither one scalar row", [](B& c, I&) { c.dims[0].num_rows = 3; });
    refused_everywhere("dims[0]: needs finite lo <= hi", [](B& c, I&) { c.dims[0].lo = 1.0; });
    refused_everywhere("overlaps", [](B& c, I&) { c.num_dims = 2; c.dims[1] = c.dims[0]; });
    // the mass configuration's own
    refused_everywhere("VineMpcAdaptInertiaConfig.abi_version", [](B&, I& m) { m.abi_version = 7; });
    refused_everywhere("num_mass_dims", [](B&, I& m) { m.num_mass_dims = 0; });
    refused_everywhere("num_mass_dims", [](B&, I& m) { m.num_mass_dims = 4; });
    refused_everywhere("unknown name", [](B&, I& m) { m.dims[0].name = 3; });
    refused_everywhere("unknown name", [](B&, I& m) { m.dims[0].name = -1; });
    refused_everywhere("repeats the name", [](B&, I& m) { m.num_mass_dims = 2; m.dims[1] = m.dims[0]; });
    refused_everywhere("lo > 0", [](B&, I& m) { m.dims[0].lo = 0.0; });
    refused_everywhere("lo > 0", [](B&, I& m) { m.dims[0].lo = -0.5; });
    refused_everywhere("finite lo <= hi", [](B&, I& m) { m.dims[0].lo = 1.5; });
    refused_everywhere("finite lo <= hi", [=](B&, I& m) { m.dims[0].hi = inf; });
    refused_everywhere("finite lo <= hi", [=](B&, I& m) { m.dims[0].lo = nan; });
    refused_everywhere("std_floor", [](B&, I& m) { m.dims[0].std_floor = -1e-3; });
    refused_everywhere("std_floor", [=](B&, I& m) { m.dims[0].std_floor = nan; });
    refused_everywhere("base_inertia", [](B&, I& m) { m.base_inertia[VI_CART_MASS] = 0.0f; });
    refused_everywhere("base_inertia", [=](B&, I& m) { m.base_inertia[VI_LINK_MASS0 + 2] = fnan; });
    refused_everywhere("base_inertia", [](B&, I& m) { m.base_inertia[VI_LINK_INERTIA0 + 4] = -1e-6f; });
    refused_everywhere("link_length", [](B&, I& m) { m.link_length = 0.0f; });
    refused_everywhere("link_com", [=](B&, I& m) { m.link_com = finf; });
    refused_everywhere("gravity", [=](B&, I& m) { m.gravity = fnan; });
    // a checked pair gets as far as the handle, whose own refusal is passed on
    refused_everywhere("stand-in handle", [](B&, I&) {});

    // null pointers
    B c = base();
    m = masses();
    alignas(8) static char buf[64];
    VineHandle* h = reinterpret_cast<VineHandle*>(buf);
    expect(pin(h, nullptr, &m, g_table) == VINE_ERR_INVALID_ARG && strstr(g_err, "mpc adapt config is NULL"), "pin(NULL config)");
    expect(pin(h, &c, nullptr, g_table) == VINE_ERR_INVALID_ARG && strstr(g_err, "mpc adapt inertia config is NULL"),
           "pin(NULL mass config)");
    expect(estimate(h, &c, nullptr, g_table) == VINE_ERR_INVALID_ARG && strstr(g_err, "mpc adapt inertia config is NULL"),
           "estimate(NULL mass config)");
    expect(pin(nullptr, &c, &m, g_table) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_adapt_inertia_pin"),
           "pin(NULL handle)");
    expect(pin(h, &c, &m, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_adapt_inertia_pin"),
           "pin(NULL table)");
    expect(vine_mpc_adapt_inertia_pin(h, &c, &m, g_table, nullptr, g_d, g_i64, nullptr) == VINE_ERR_INVALID_ARG &&
               strstr(g_err, "null argument"), "pin(NULL mean)");
    expect(estimate(h, &c, &m, nullptr) == VINE_ERR_INVALID_ARG && strstr(g_err, "null argument to vine_mpc_adapt_inertia_estimate"),
           "estimate(NULL table)");
    expect(vine_mpc_adapt_inertia_estimate(h, &c, &m, g_table, nullptr, g_i32, g_u8, g_d, g_d, g_d, g_d, g_i64, nullptr, nullptr) ==
               VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "estimate(NULL err)");
    expect(vine_mpc_adapt_inertia_estimate(h, &c, &m, g_table, g_d, g_i32, g_u8, g_d, g_d, g_d, nullptr, g_i64, nullptr, nullptr) ==
               VINE_ERR_INVALID_ARG && strstr(g_err, "null argument"), "estimate(NULL prior std)");

    // the handle: N != M K, no inertia table bound, another one bound than the memory passed
    static float other[4];
    g_envs = 47;
    g_params = other;
    g_inertia = g_table;
    expect(pin(h, &c, &m, g_table) == VINE_ERR_INVALID_ARG && strstr(g_err, "has 47 envs, not num_plants * samples = 3 * 16"),
           "pin(N != M K)");
    expect(estimate(h, &c, &m, g_table) == VINE_ERR_INVALID_ARG && strstr(g_err, "has 47 envs"), "estimate(N != M K)");
    g_envs = 48;
    g_inertia = nullptr;
    expect(pin(h, &c, &m, g_table) == VINE_ERR_UNSUPPORTED && strstr(g_err, "no inertia table bound"), "pin(no inertia table)");
    expect(estimate(h, &c, &m, g_table) == VINE_ERR_UNSUPPORTED && strstr(g_err, "no inertia table bound"),
           "estimate(no inertia table)");
    g_inertia = other;
    expect(pin(h, &c, &m, g_table) == VINE_ERR_UNSUPPORTED && strstr(g_err, "is not the table bound"), "pin(other memory)");
    expect(estimate(h, &c, &m, g_table) == VINE_ERR_UNSUPPORTED && strstr(g_err, "is not the table bound"),
           "estimate(other memory)");

    if (failures) return 1;
    printf("mpc adapt inertia host check ok\n");
    return 0;
}
