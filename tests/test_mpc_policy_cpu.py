"""MPC_POLICY without a GPU: the C ABI of include/vine_mpc_policy.h against its ctypes mirror, every refusal of the library that
comes before a handle is looked at and every ``ConfigError`` by name, the build plumbing of the thirteenth unit, and the numpy
statements (``head``, ``act``, ``keep``, ``terminal``, ``compose``) on hand-made rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_policy
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "vine_mpc_policy.h")).read()


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


# (name, handles, pointer-or-scalar arguments behind the two configurations, the stream included)
ENTRY_POINTS = (("vine_mpc_policy_fork", 2, 11), ("vine_mpc_policy_act", 1, 13), ("vine_mpc_policy_terminal", 1, 10),
                ("vine_mpc_policy_compose", 1, 5))


def _configs(**over):
    c = mpc.mpc_config(over.pop("num_plants", 2), over.pop("samples", 256), over.pop("horizon", 3))
    for k in ("abi_version",):
        if "mpc_" + k in over:
            setattr(c, k, over.pop("mpc_" + k))
    pc = mpc_policy.policy_config(26)
    for k, v in over.items():
        setattr(pc, k, v)
    return c, pc


def _calls(lib, c, pc):
    out = []
    for name, handles, rest in ENTRY_POINTS:
        args = [None] * handles + [c, pc]
        if name == "vine_mpc_policy_fork":
            args += [None, 26, None, 26, None, None, None, None, None, 352, None]
        else:
            args += [None] * rest
        out.append((name, getattr(lib, name), args))
    return out


# --------------------------------------------------------------------------------------------------------------- ABI
def test_policy_header_and_ctypes_mirror_agree(hip_lib):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(vine_mpc_policy_[a-z_0-9]+)\s*\(", code)))
    assert names == sorted(abi.MPC_POLICY_PROTOTYPES) and len(names) == 6
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_mpc_policy_config_size() == C.sizeof(abi.VineMpcPolicyConfig) == 4 + 4 + 4 + 4 + 8
    body = re.search(r"typedef struct VineMpcPolicyConfig \{(.*?)\} VineMpcPolicyConfig;", code, re.S).group(1)
    fields = re.findall(r"^\s+(?:int32_t|float|double)\s+([a-z_]+);", body, re.M)
    assert fields == [n for n, _ in abi.VineMpcPolicyConfig._fields_]
    for macro, value in (("ABI_VERSION", abi.MPC_POLICY_ABI_VERSION), ("UNITS", abi.MPC_POLICY_UNITS),
                         ("ROWS", abi.MPC_POLICY_ROWS)):
        assert int(re.search(r"#define VINE_MPC_POLICY_%s (\d+)" % macro, text).group(1)) == value
    for name, handles, rest in ENTRY_POINTS:
        decl = re.search(r"int %s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(abi.MPC_POLICY_PROTOTYPES[name][1]) == handles + 2 + rest, name
    for other in ("vine.h", "vine_mpc.h", "vine_mpc_adapt.h"):
        assert "vine_mpc_policy" not in open(os.path.join(REPO, "include", other)).read(), other
    assert not set(abi.MPC_POLICY_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.MPC_PROTOTYPES) | set(abi.MPC_ADAPT_PROTOTYPES))


def test_policy_defaults(hip_lib):
    pc = abi.VineMpcPolicyConfig()
    assert hip_lib.vine_mpc_policy_config_default(pc) == abi.OK
    assert (pc.abi_version, pc.obs_width, pc.terminal_value) == (1, 0, 0.0)
    assert pc.ln_eps == np.float32(mpc_policy.DEFAULTS["ln_eps"]) and pc.value_eps == np.float32(mpc_policy.DEFAULTS["value_eps"])
    assert hip_lib.vine_mpc_policy_config_default(None) == abi.ERR_INVALID_ARG
    assert b"config is NULL" in hip_lib.vine_last_error()


def test_policy_build_plumbing():
    assert native.LIB_UNITS == native.ALL_UNITS + (native.SRC_MPC_ADAPT,) and len(native.LIB_UNITS) == 12      # still pinned
    assert native.POLICY_UNITS == native.LIB_UNITS + (native.SRC_MPC_POLICY,) and len(native.POLICY_UNITS) == 13
    assert native.SRC_MPC_POLICY not in native.LIB_UNITS
    assert os.path.basename(native.SRC_MPC_POLICY) == "vine_mpc_policy.hip" and os.path.exists(native.SRC_MPC_POLICY)
    deps = [os.path.basename(d) for d in native.DEPS]
    for name in ("vine_mpc_policy.hip", "vine_mpc_policy.h", "vine_mpc.h", "vine_policy_head.h", "vine_task_shared.h"):
        assert name in deps, name
    assert any(d.endswith("vine_mpc_policy.h") for d in native._SOURCE_HEADERS[native.SRC_MPC_POLICY])
    assert native._SOURCE_FLAGS[native.SRC_MPC_POLICY] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_MPC_POLICY)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast")
    src = open(native.SRC_MPC_POLICY).read()
    assert src.index("#pragma clang fp contract(off)") < src.index("#include")
    # contraction is on again exactly around the head and the step's own clamp
    on = src.index("#pragma clang fp contract(fast)")
    off_again = src.index("#pragma clang fp contract(off)", on)
    between = [line for line in src[on:off_again].splitlines()[1:] if line.strip()]
    assert between == ['#include "vine_policy_head.h"', '#include "vine_task_shared.h"']
    assert "quad_ln_heads<3>" in src and "unnormalize_value(" in src
    assert "atomic" not in re.sub(r"//.*", "", src) and "__shared__" not in src
    # build() compiles and links the new tuple
    import inspect
    assert "for src in POLICY_UNITS" in inspect.getsource(native.build)


# ------------------------------------------------------------------------------------------------- the library's refusals
@pytest.mark.parametrize("over, word", [
    (dict(mpc_abi_version=7), b"VineMpcConfig.abi_version"), (dict(abi_version=7), b"VineMpcPolicyConfig.abi_version"),
    (dict(samples=255), b"multiple of 512"), (dict(num_plants=1), b"multiple of 512"), (dict(num_plants=3, samples=256), b"multiple of 512"),
    (dict(obs_width=0), b"obs_width"), (dict(obs_width=abi.MAX_OBS + 1), b"obs_width"),
    (dict(ln_eps=float("nan")), b"ln_eps"), (dict(ln_eps=-1e-5), b"ln_eps"), (dict(value_eps=float("inf")), b"value_eps"),
    (dict(terminal_value=-0.5), b"terminal_value"), (dict(terminal_value=float("inf")), b"terminal_value"),
    (dict(terminal_value=float("nan")), b"terminal_value")])
def test_policy_refuses_bad_configs(hip_lib, over, word):
    """Validation comes before the handles or any pointer is looked at, so no device is needed to see it."""
    c, pc = _configs(**over)
    for name, fn, args in _calls(hip_lib, c, pc):
        hip_lib.vine_set_step_count(None, -1)             # leaves another message behind
        assert fn(*args) == abi.ERR_INVALID_ARG, name
        assert word in hip_lib.vine_last_error(), hip_lib.vine_last_error()


def test_policy_refuses_null_pointers_and_null_configs(hip_lib):
    for c, pc in (_configs(), _configs(num_plants=3, samples=512, terminal_value=2.0)):
        for name, fn, args in _calls(hip_lib, c, pc):
            assert fn(*args) == abi.ERR_INVALID_ARG
            assert b"null argument to " + name.encode() in hip_lib.vine_last_error(), hip_lib.vine_last_error()
    c, pc = _configs()
    for name, fn, args in _calls(hip_lib, None, pc):
        assert fn(*args) == abi.ERR_INVALID_ARG and b"mpc config is NULL" in hip_lib.vine_last_error()
    for name, fn, args in _calls(hip_lib, c, None):
        assert fn(*args) == abi.ERR_INVALID_ARG and b"mpc policy config is NULL" in hip_lib.vine_last_error()


def test_policy_refuses_widths_and_misaligned_rows(hip_lib):
    """Past the null checks and still in front of the handles: host memory stands in for the buffers (nothing is read)."""
    c, pc = _configs()
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) // 16 * 16
    h1, h2, p, odd8, odd4 = base, base + 64, base + 16, base + 24, base + 20
    lib = hip_lib

    def refused(fn, args, word):
        lib.vine_set_step_count(None, -1)
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert word in lib.vine_last_error(), lib.vine_last_error()

    fork = lib.vine_mpc_policy_fork
    refused(fork, [h1, h2, c, pc, p, 26, p, 14, p, p, p, p, p, 352, None], b"observation width")
    refused(fork, [h1, h2, c, pc, p, 14, p, 14, p, p, p, p, p, 352, None], b"observation width")
    refused(fork, [h1, h2, c, pc, p, 26, p, 26, odd8, p, p, p, p, 352, None], b"16-byte aligned")
    refused(fork, [h1, h2, c, pc, p, 26, p, 26, p, p, p, p, odd8, 352, None], b"16-byte aligned")
    refused(fork, [h1, h2, c, pc, p, 26, p, 26, p, p, p, p, p, 354, None], b"16-byte aligned")
    refused(fork, [h1, h2, c, pc, p, 26, p, 26, p, p, p, p, p, 252, None], b"16-byte aligned")
    refused(fork, [h1, h1, c, pc, p, 26, p, 26, p, p, p, p, p, 352, None], b"two handles")
    act = lib.vine_mpc_policy_act
    refused(act, [h1, c, pc, odd8, p, p, p, p, p, p, p, p, p, p, None, None], b"16-byte aligned")
    refused(act, [h1, c, pc, p, p, p, p, p, p, p, odd4, p, p, p, None, None], b"8-byte aligned")
    refused(act, [h1, c, pc, p, p, p, p, p, p, p, p, odd4, p, p, None, None], b"8-byte aligned")
    refused(act, [h1, c, pc, p, p, p, p, p, p, p, p, p, p, p, odd4, None], b"8-byte aligned")
    term = lib.vine_mpc_policy_terminal
    refused(term, [h1, c, pc, p, p, p, p, None, p, p, p, None, None], b"both or neither")
    refused(term, [h1, c, pc, p, odd8, p, p, p, p, p, p, None, None], b"16-byte aligned")
    refused(lib.vine_mpc_policy_compose, [h1, c, pc, p, p, odd4, p, None], b"8-byte aligned")
    refused(lib.vine_mpc_policy_compose, [h1, c, pc, p, p, p, odd4, None], b"8-byte aligned")


# ------------------------------------------------------------------------------------------------------- policy_config
def test_policy_config_fills_the_mirror():
    pc = mpc_policy.policy_config(26, 1e-5, 1e-5, 0.75)
    assert (pc.abi_version, pc.obs_width, pc.terminal_value) == (abi.MPC_POLICY_ABI_VERSION, 26, 0.75)
    assert pc.ln_eps == np.float32(1e-5) and pc.value_eps == np.float32(1e-5)
    assert mpc_policy.policy_config(1).terminal_value == 0.0 and mpc_policy.policy_config(abi.MAX_OBS).obs_width == abi.MAX_OBS


@pytest.mark.parametrize("kw, word", [
    (dict(obs_width=0), "obs_width"), (dict(obs_width=abi.MAX_OBS + 1), "obs_width"), (dict(obs_width=2.5), "obs_width"),
    (dict(obs_width=True), "obs_width"), (dict(ln_eps=-1.0), "ln_eps"), (dict(ln_eps=float("nan")), "ln_eps"),
    (dict(ln_eps="x"), "ln_eps"), (dict(value_eps=float("inf")), "value_eps"), (dict(value_eps=-1e-9), "value_eps"),
    (dict(terminal_value=-0.1), "terminal_value"), (dict(terminal_value=float("nan")), "terminal_value"),
    (dict(terminal_value=float("inf")), "terminal_value"), (dict(terminal_value=None), "terminal_value"),
    (dict(terminal_value=True), "terminal_value")])
def test_policy_config_errors_name_the_key(kw, word):
    args = dict(obs_width=26)
    args.update(kw)
    with pytest.raises(ConfigError, match=re.escape("mpc policy: " + word)):
        mpc_policy.policy_config(**args)


def test_shape_and_play_refusals_name_the_reason():
    assert mpc_policy.check_shape(2, 256) == 512 and mpc_policy.check_shape(3, 512) == 1536
    for m, k in ((4, 64), (1, 256), (3, 256), (2, 255)):
        with pytest.raises(ConfigError, match="multiple of 512"):
            mpc_policy.check_shape(m, k)
    cfg = {"env": {"numEnvs": 2}, "seed": 0}
    # refused before any task is created (no device needed)
    with pytest.raises(ConfigError, match="terminal_value needs policy="):
        mpc.play(cfg, samples=256, terminal_value=1.0)
    with pytest.raises(ConfigError, match="policy= together with adapt= is refused"):
        mpc.play(cfg, samples=256, policy="x.pth", adapt={"params": {"DAMPING": [0.005, 0.1]}}, policy_params={})
    with pytest.raises(ConfigError, match="policy= needs policy_params"):
        mpc.play(cfg, samples=256, policy="x.pth")
    with pytest.raises(ConfigError, match="multiple of 512"):
        mpc.play(cfg, samples=64, policy="x.pth", policy_params={})
    with pytest.raises(ConfigError, match="mpc policy: terminal_value"):
        mpc.play(cfg, samples=256, policy="x.pth", policy_params={}, terminal_value=-1.0)


# ------------------------------------------------------------------------------------------------- the numpy statements
def test_head_is_the_layernorm_and_the_three_rows():
    rng = np.random.default_rng(0)
    y = rng.normal(0.3, 2.0, (5, 256)).astype(np.float32)
    gamma, beta = 1.0 + 0.1 * rng.normal(size=256), 0.1 * rng.normal(size=256)
    w, b = 0.1 * rng.normal(size=(3, 256)), 0.1 * rng.normal(size=3)
    hw, hc = gamma * w, w @ beta + b                          # vine_rollout_head_prep's products
    out = mpc_policy.head(y, hw, hc, 1e-5)
    assert out.shape == (5, 3) and out.dtype == np.float64
    y64 = y.astype(np.float64)
    ln = (y64 - y64.mean(1, keepdims=True)) / np.sqrt(y64.var(1, keepdims=True) + 1e-5) * gamma + beta
    assert np.allclose(out, ln @ w.T + b, rtol=1e-12, atol=1e-12)
    const = mpc_policy.head(np.full((1, 256), 3.0), hw, hc)   # a constant row: the LayerNorm gives beta
    assert np.allclose(const, hc, rtol=0, atol=1e-9)


def test_act_is_one_add_and_the_clamp_at_both_ends():
    mu = np.float32([[0.25, -0.5], [0.9, -0.9], [0.1, 0.2], [1e-8, 0.0]])
    d = np.float32([[0.5, 0.25], [0.3, -0.3], [-0.1, -0.2], [1.0, -1.0]])
    a = mpc_policy.act(mu, d, 1.0)
    assert a.dtype == np.float32
    assert np.array_equal(a, np.float32([[0.75, -0.25], [1.0, -1.0], [0.0, 0.0], [1.0, -1.0]]))
    assert np.array_equal(mpc_policy.act(mu, d, 0.5), np.float32([[0.5, -0.25], [0.5, -0.5], [0.0, 0.0], [0.5, -0.5]]))
    # one float32 rounding: the sum is formed in float32, not in float64 and rounded behind the clamp
    x, y = np.float32(0.1), np.float32(0.2)
    assert mpc_policy.act([[x, x]], [[y, y]], 1.0)[0, 0] == x + y
    assert np.array_equal(mpc_policy.act(mu, np.zeros_like(mu), 1.0), mu)        # a zero perturbation: the policy itself


def test_keep_takes_sample_zero_and_zeroes_a_plant_whose_reset_is_raised():
    M, K = 3, 4
    rng = np.random.default_rng(1)
    mu = rng.normal(size=(M * K, 2)).astype(np.float32)
    h, c = rng.normal(size=(M * K, 256)).astype(np.float32), rng.normal(size=(M * K, 256)).astype(np.float32)
    mu0, ph, pc = mpc_policy.keep(mu, h, c, K)
    assert np.array_equal(mu0, mu[[0, 4, 8]]) and np.array_equal(ph, h[[0, 4, 8]]) and np.array_equal(pc, c[[0, 4, 8]])
    mu0, ph, pc = mpc_policy.keep(mu, h, c, K, plant_reset=[0, 1, 0])
    assert np.array_equal(mu0[[0, 2]], mu[[0, 8]]) and np.array_equal(ph[[0, 2]], h[[0, 8]]) and np.array_equal(pc[2], c[8])
    assert not mu0[1].any() and not ph[1].any() and not pc[1].any()
    assert mu.any() and h[4].any()                                                # (the inputs were not written)


def test_terminal_on_an_alive_a_dead_and_a_nan_sample():
    cost = np.array([1.0, 2.0, 3.0, np.inf, 0.5])
    alive = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    v = np.float32([0.5, 100.0, np.nan, 1.0, -np.inf])
    out, live = mpc_policy.terminal(cost, alive, v, 2.0)
    assert out[0] == 1.0 - 2.0 * 0.5 and live[0] == 1
    assert out[1] == 2.0 and live[1] == 0                                         # a dead sample is not touched
    assert np.isposinf(out[2]) and live[2] == 0                                   # a NaN value: +inf, no longer alive
    assert np.isposinf(out[3]) and live[3] == 0
    assert np.isposinf(out[4]) and live[4] == 0                                   # -inf is not finite either
    assert out.dtype == np.float64 and live.dtype == np.uint8
    # one float64 multiply, one subtract, from the float32 value
    w, val = 0.3, np.float32(0.7)
    assert mpc_policy.terminal([0.1], [1], [val], w)[0][0] == 0.1 - np.float64(w) * np.float64(val)
    same, _ = mpc_policy.terminal(cost, alive, v, 0.0)
    assert same[0] == 1.0 and same[1] == 2.0
    assert cost[2] == 3.0                                                         # (the input was not written)


def test_unnormalize_value_is_the_normalisers_float32_arithmetic():
    v = np.float32([0.5, 7.0, -9.0])
    got = mpc_policy.unnormalize_value(v, 0.37, 2.3, 1e-5)
    std = np.sqrt(np.float32(2.3) + np.float32(1e-5))
    assert got.dtype == np.float32
    assert np.array_equal(got, np.float32([0.5, 5.0, -5.0]) * std + np.float32(0.37))


def test_compose_clamps_at_both_ends_and_leaves_a_plant_whose_reset_is_raised():
    mu0 = np.float32([[0.5, -0.5], [0.9, -0.9], [0.3, 0.3], [0.2, 0.1]])
    residual = np.float32([[0.25, 0.25], [0.5, -0.5], [0.0, 0.0], [0.1, 0.1]])
    history = np.arange(4 * abi.MAX_DELAY * 2, dtype=np.float32).reshape(4, abi.MAX_DELAY, 2)
    history[:, 0] = residual                                                     # the update wrote the residual's first entry
    history[2, 0] = 0.0
    a, hist = mpc_policy.compose(mu0, residual, history, 1.0, plant_reset=[0, 0, 1, 0])
    assert np.array_equal(a, np.float32([[0.75, -0.25], [1.0, -1.0], [0.0, 0.0], [np.float32(0.2) + np.float32(0.1), 0.2]]))
    assert np.array_equal(hist[:, 0], a)                                          # what the plant really receives
    assert np.array_equal(hist[:, 1:], history[:, 1:])
    a2, hist2 = mpc_policy.compose(mu0, residual, history, 1.0)
    assert np.array_equal(a2[2], mu0[2]) and np.array_equal(hist2[:, 0], a2)
    assert np.array_equal(history[1, 0], residual[1])                             # (the input was not written)
