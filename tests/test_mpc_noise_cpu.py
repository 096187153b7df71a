"""MPC_NOISE without a GPU: include/vine_mpc_noise.h against its ctypes mirror and the build plumbing of the nineteenth unit,
every ``ConfigError`` of ``noise_config`` and ``Play``'s refusal of the five other variants, every refusal of the entry points
by name through the library and through the stand-alone scripts/mpc_noise_host_check.cpp (built with the host's sanitizers),
and the numpy statements of utils/mpc_noise.py: ``colored_deviate`` against the base deviate and its statistics, ``noise_replay``
on hand-made costs."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_sensor, mpc, mpc_noise
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError, parse_scalar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
K0 = env_sensor.NOISE_SCALE


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_the_struct_size_and_the_build_wiring(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_mpc_noise.h")).read(), flags=re.S)
    for macro, value in (("VINE_MPC_NOISE_ABI_VERSION", abi.MPC_NOISE_ABI_VERSION), ("VINE_MPC_NOISE_THREADS", abi.MPC_NOISE_THREADS)):
        assert int(re.search(r"#define %s (\d+)\s" % macro, text).group(1)) == value, macro
    assert abi.MPC_NOISE_THREADS == abi.MPC_THREADS == 256
    body = re.search(r"typedef struct VineMpcNoiseConfig \{(.*?)\} VineMpcNoiseConfig;", text, flags=re.S).group(1)
    decls = [decl.strip() for decl in body.split(";") if decl.strip()]
    fields = [re.sub(r"\[.*?\]", "", d).split()[-1] for d in decls]
    assert fields == [f[0] for f in abi.VineMpcNoiseConfig._fields_]
    assert fields == ["abi_version", "beta", "adapt", "rate", "sigma_min", "sigma_max"]
    kinds = {"int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}
    for d, (name, ctype) in zip(decls, abi.VineMpcNoiseConfig._fields_):
        base = kinds[d.split()[0]]
        assert ctype == (base * 2 if "[2]" in d else base), name
    assert lib.vine_mpc_noise_config_size() == C.sizeof(abi.VineMpcNoiseConfig) == 40
    functions = sorted(set(re.findall(r"\b(vine_mpc_noise[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.MPC_NOISE_PROTOTYPES) and len(functions) == 5
    for name in functions:
        assert hasattr(lib, name), name
    for name, count in (("vine_mpc_noise_draw", 6), ("vine_mpc_noise_scheduled", 9), ("vine_mpc_noise_update", 13)):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(decl.split(",")) == len(abi.MPC_NOISE_PROTOTYPES[name][1]) == count, name
    assert "declare_mpc_noise" in inspect.getsource(abi.declare_all)
    c = abi.VineMpcNoiseConfig()
    assert lib.vine_mpc_noise_config_default(C.byref(c)) == abi.OK
    assert (c.abi_version, list(c.beta), c.adapt, c.rate, list(c.sigma_min)) == (1, [0.0, 0.0], 0, 0.2, [0.0, 0.0])
    assert list(c.sigma_max) == [float(np.finfo(f32).max)] * 2
    # nothing of it went into the base header, whose functions an existing test counts
    assert "mpc_noise" not in open(os.path.join(REPO, "include", "vine_mpc.h")).read()


def test_the_pinned_unit_tuples_stand_and_the_new_unit_is_built():
    n = native
    assert n.BUILD_UNITS == n.UNITS + (n.SRC_PUSH,) and n.ALL_UNITS == n.BUILD_UNITS + (n.SRC_MPC,)
    assert n.LIB_UNITS == n.ALL_UNITS + (n.SRC_MPC_ADAPT,) and n.POLICY_UNITS == n.LIB_UNITS + (n.SRC_MPC_POLICY,)
    assert len(n.UNITS) == 9 and len(n.POLICY_UNITS) == 13 and n.LATER_UNITS == (n.SRC_DRAW_ADR,)
    assert n.NOISE_UNITS == (n.SRC_MPC_NOISE,)
    for pinned in (n.SOURCES, n.UNITS, n.BUILD_UNITS, n.ALL_UNITS, n.LIB_UNITS, n.POLICY_UNITS, n.LATER_UNITS):
        assert n.SRC_MPC_NOISE not in pinned
    build = inspect.getsource(n.build)
    assert "map(compile_unit, LATER_UNITS)" in build and "map(compile_unit, NOISE_UNITS)" in build
    assert build.index("map(compile_unit, LATER_UNITS)") < build.index("map(compile_unit, NOISE_UNITS)") < build.index("proc.wait()")
    assert build.count("compile_unit(") == 3
    assert os.path.basename(n.SRC_MPC_NOISE) == "vine_mpc_noise.hip" and os.path.exists(n.SRC_MPC_NOISE)
    assert n.SRC_MPC_NOISE in n.DEPS and any(d.endswith("vine_mpc_noise.h") for d in n.DEPS)
    headers = {os.path.basename(h) for h in n._SOURCE_HEADERS[n.SRC_MPC_NOISE]}
    assert {"vine_mpc.h", "vine_mpc_noise.h", "vine_mpc_shared.h"} <= headers
    assert n._SOURCE_FLAGS[n.SRC_MPC_NOISE] == ["-ffp-contract=fast-honor-pragmas"]
    flags = n._flags(n.SRC_MPC_NOISE)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast") and "-ffp-contract=off" not in flags
    source = open(n.SRC_MPC_NOISE).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    assert "atomic" not in source.replace("No atomics", "").replace("no atomics", "") and "hipMalloc" not in source
    assert "Synchronize" not in source and '#include "vine_mpc_shared.h"' in source
    # the base unit knows nothing of it
    for other in (n.SRC, n.SRC_PPO, n.SRC_MPC):
        assert "mpc_noise" not in open(other).read().lower(), other


# ------------------------------------------------------------------------------------------------------ the configuration
def test_every_config_error_of_noise_config_by_name():
    assert mpc_noise.noise_config({"BETA": 0.8}) == {"BETA": [0.8, 0.8], "ADAPT": None}
    got = mpc_noise.noise_config(parse_scalar("{BETA: [0.9, 0.7], ADAPT: {RATE: 0.2, SIGMA_MIN: 0.05, SIGMA_MAX: 1.0}}"))
    assert got == {"BETA": [0.9, 0.7], "ADAPT": {"RATE": 0.2, "SIGMA_MIN": [0.05, 0.05], "SIGMA_MAX": [1.0, 1.0]}}
    assert mpc_noise.noise_config(got) == got
    assert mpc_noise.noise_config({"BETA": 0, "ADAPT": {}})["ADAPT"] == {"RATE": 0.2, "SIGMA_MIN": [0.05] * 2, "SIGMA_MAX": [1.0] * 2}
    with pytest.raises(ConfigError, match="noise=.*must be a mapping, not 0.8"):
        mpc_noise.noise_config(0.8)
    with pytest.raises(ConfigError, match=r"noise: unknown key\(s\) Beta, RATE"):
        mpc_noise.noise_config({"BETA": 0.5, "RATE": 0.1, "Beta": 1})
    with pytest.raises(ConfigError, match="noise.BETA is missing"):
        mpc_noise.noise_config({})
    for bad in (1.0, -0.1, 1.5, 0.99999999):
        with pytest.raises(ConfigError, match=r"noise.BETA must lie in \[0, 1\)"):
            mpc_noise.noise_config({"BETA": bad})
    for bad in ("0.8", None, True, float("nan"), float("inf")):
        with pytest.raises(ConfigError, match="noise.BETA: .* is not a finite number"):
            mpc_noise.noise_config({"BETA": bad})
    with pytest.raises(ConfigError, match="noise.BETA is one number or two"):
        mpc_noise.noise_config({"BETA": [0.1, 0.2, 0.3]})
    with pytest.raises(ConfigError, match="noise.ADAPT=.*must be a mapping, not True"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": True})
    with pytest.raises(ConfigError, match=r"noise.ADAPT: unknown key\(s\) rate"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"rate": 0.5}})
    for bad in (0.0, -0.5, 1.01):
        with pytest.raises(ConfigError, match=r"noise.ADAPT.RATE must lie in \(0, 1\]"):
            mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"RATE": bad}})
    with pytest.raises(ConfigError, match="noise.ADAPT.RATE: .* is not a finite number"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"RATE": "fast"}})
    with pytest.raises(ConfigError, match="noise.ADAPT.SIGMA_MIN must not be negative"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"SIGMA_MIN": [0.1, -0.1]}})
    with pytest.raises(ConfigError, match="noise.ADAPT.SIGMA_MAX: .* is not a finite number"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"SIGMA_MAX": float("inf")}})
    with pytest.raises(ConfigError, match="noise.ADAPT.SIGMA_MAX must fit a float32"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"SIGMA_MAX": 1e39}})
    with pytest.raises(ConfigError, match="noise.ADAPT.SIGMA_MIN is one number or two"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"SIGMA_MIN": []}})
    with pytest.raises(ConfigError, match="noise.ADAPT.SIGMA_MIN 0.5 lies above SIGMA_MAX 0.4"):
        mpc_noise.noise_config({"BETA": 0.5, "ADAPT": {"SIGMA_MIN": 0.5, "SIGMA_MAX": 0.4}})
    # the struct beside a controller's configuration
    mcfg = mpc.mpc_config(3, 16, 5, sigma=[0.5, 0.25])
    c = mpc_noise.noise_struct({"BETA": [0.9, 0.7], "ADAPT": {"RATE": 0.3, "SIGMA_MIN": 0.05, "SIGMA_MAX": [1.0, 0.5]}}, mcfg)
    assert (c.abi_version, c.adapt, c.rate) == (abi.MPC_NOISE_ABI_VERSION, 1, 0.3)
    assert list(c.beta) == [float(f32(0.9)), float(f32(0.7))] and list(c.sigma_max) == [1.0, 0.5]
    c = mpc_noise.noise_struct({"BETA": 0.8}, mpc.mpc_config(3, 16, 5, sigma=40.0))      # no ADAPT: no bound on sigma
    assert c.adapt == 0 and list(c.sigma_min) == [0.0, 0.0] and list(c.sigma_max) == [float(np.finfo(f32).max)] * 2
    for sigma in (0.01, [0.5, 1.5]):
        with pytest.raises(ConfigError, match="noise.ADAPT: sigma .* lies outside SIGMA_MIN .. SIGMA_MAX"):
            mpc_noise.noise_struct({"BETA": 0.8, "ADAPT": {}}, mpc.mpc_config(3, 16, 5, sigma=sigma))


OTHER_ARGUMENT = {"track": {"PATH": "exact"}, "observe": {"DELAY": 1}, "filter": {}, "adapt": {"params": {"DAMPING": [0.005, 0.1]}},
                  "policy": "x.pth"}


@pytest.mark.parametrize("other", mpc_noise.OTHERS)
def test_play_refuses_noise_together_with_each_other_variant_by_name(other, monkeypatch):
    assert mpc_noise.OTHERS == ("track", "observe", "filter", "policy", "adapt")
    message = "mpc: noise= together with %s= is refused" % other
    args = dict.fromkeys(mpc.VARIANTS)
    args.update({"noise": {"BETA": 0.8}, other: OTHER_ARGUMENT[other]})
    run = types.SimpleNamespace(args=args, M=2, samples=16, planner=(5, 0.05, 0.5, 0))
    with pytest.raises(ConfigError, match=message):
        mpc_noise.Play({"BETA": 0.8}).check(run)
    # ... and through play, before any task is made (filter needs observe beside it: the table of rules comes first)

    def no_task(*a, **k):
        raise AssertionError("a task was made before the combination was refused")

    monkeypatch.setattr(mpc, "make_task", no_task)
    env = {"numEnvs": 2, "ENV_TARGET": {"VEL_ALONG": 0.1, "SPAN_ALONG": 0.05}}
    given = {other: OTHER_ARGUMENT[other]}
    if other == "filter":
        given["observe"], message = OTHER_ARGUMENT["observe"], "mpc: noise= together with observe= is refused"
    with pytest.raises(ConfigError, match=message):
        mpc.play({"env": env, "seed": 0}, samples=256, noise={"BETA": 0.8}, **given)


def test_play_takes_noise_and_the_rule_table_is_unchanged(monkeypatch):
    assert mpc.VARIANTS == ("noise", "track", "observe", "filter", "policy", "adapt")
    assert inspect.signature(mpc.play).parameters["noise"].default is None
    assert len(mpc.RULES) == 12 and not any("noise" in k for keys, _ in mpc.RULES for k in keys)
    assert not any("noise" in message for _, message in mpc.RULES)
    import mpc as tool
    assert tool.OWN["noise"] is None and "noise=own[\"noise\"]" in inspect.getsource(tool.main)
    with pytest.raises(ConfigError, match="mpc: noise=.*must be a mapping, not 0.8"):
        tool.main(["noise=0.8"])
    plain = {"env": {"numEnvs": 2}, "seed": 0}
    with pytest.raises(ConfigError, match=r"noise.BETA must lie in \[0, 1\)"):
        mpc.play(plain, samples=16, noise={"BETA": 1.0})
    with pytest.raises(ConfigError, match="noise.ADAPT: sigma 2 lies outside"):
        mpc.play(plain, samples=16, sigma=2.0, noise={"BETA": 0.5, "ADAPT": {}})


# ------------------------------------------------------------------------------------------- refusals of the entry points
def _configs(lib, **noise):
    mcfg = mpc.mpc_config(3, 16, 5)
    n = abi.VineMpcNoiseConfig()
    assert lib.vine_mpc_noise_config_default(C.byref(n)) == abi.OK
    for k, v in noise.items():
        if isinstance(v, (list, tuple)):
            getattr(n, k)[0], getattr(n, k)[1] = v
        else:
            setattr(n, k, v)
    return mcfg, n


REFUSALS = (
    ("VineMpcNoiseConfig.abi_version mismatch", dict(abi_version=2)),
    ("mpc noise beta must be finite and in [0, 1)", dict(beta=[1.0, 0.0])),
    ("mpc noise beta must be finite and in [0, 1)", dict(beta=[0.0, -0.25])),
    ("mpc noise beta must be finite and in [0, 1)", dict(beta=[float("nan"), 0.0])),
    ("mpc noise rate must be in (0, 1] with adapt", dict(adapt=1, rate=0.0)),
    ("mpc noise rate must be in (0, 1] with adapt", dict(adapt=1, rate=1.25)),
    ("mpc noise rate must be in (0, 1] with adapt", dict(adapt=1, rate=float("nan"))),
    ("mpc noise sigma_min must be finite and not negative", dict(sigma_min=[-0.1, 0.0])),
    ("mpc noise sigma_min must be finite and not negative", dict(sigma_min=[0.0, float("inf")])),
    ("mpc noise sigma_max must be finite", dict(sigma_max=[float("inf"), 1.0])),
    ("mpc noise sigma_max must be finite", dict(sigma_max=[1.0, float("nan")])),
    ("mpc noise needs sigma_min <= sigma <= sigma_max, sigma of the VineMpcConfig", dict(sigma_min=[0.6, 0.0])),
    ("mpc noise needs sigma_min <= sigma <= sigma_max, sigma of the VineMpcConfig", dict(sigma_max=[1.0, 0.4])),
    ("null argument to vine_mpc_noise_", dict(rate=9.0)),                       # without adapt the rate is not looked at
    ("null argument to vine_mpc_noise_", dict()),
)


@pytest.mark.parametrize("message,change", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_of_the_entry_points_by_name(lib, message, change):
    mcfg, n = _configs(lib, **change)
    calls = (lambda: lib.vine_mpc_noise_draw(None, mcfg, n, None, None, None),
             lambda: lib.vine_mpc_noise_scheduled(None, mcfg, n, None, None, None, None, None, None),
             lambda: lib.vine_mpc_noise_update(None, mcfg, n, None, None, None, None, None, None, None, None, None, None))
    for call in calls:
        assert call() == abi.ERR_INVALID_ARG
        assert message in lib.vine_last_error().decode()
    # the base configuration is refused first, in vine_mpc.hip's words
    mcfg.horizon = abi.MPC_MAX_HORIZON + 1
    for call in calls:
        assert call() == abi.ERR_INVALID_ARG
        assert lib.vine_last_error() == b"mpc needs 1 <= horizon <= VINE_MPC_MAX_HORIZON (64)"
    assert lib.vine_mpc_noise_draw(None, None, n, None, None, None) == abi.ERR_INVALID_ARG
    assert lib.vine_last_error() == b"mpc config is NULL"
    assert lib.vine_mpc_noise_draw(None, mpc.mpc_config(3, 16, 5), None, None, None, None) == abi.ERR_INVALID_ARG
    assert lib.vine_last_error() == b"mpc noise config is NULL"
    assert lib.vine_mpc_noise_config_default(None) == abi.ERR_INVALID_ARG


def test_the_refusals_through_the_stand_alone_host_check(tmp_path):
    """scripts/mpc_noise_host_check.cpp, built as its head says -- the unit's HOST code under AddressSanitizer and UBSan, with a
    stand-in handle -- walks every refusal by name, the misaligned buffers and the handle's own refusal included.  A few seconds
    of hipcc.  Nothing is loaded into Python under a sanitizer."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "mpc_noise_host_check")
    source = os.path.join(REPO, "scripts", "mpc_noise_host_check.cpp")
    text = open(source).read()
    for word in ('"beta"', '"rate"', '"sigma_min"', '"sigma_max"', '"sigma_min <= sigma <= sigma_max"', "8-byte aligned",
                 "mpc noise config is NULL", '"null argument"', "stand-in handle"):
        assert word in text, word
    subprocess.check_call([hipcc, "--offload-arch=" + native.ARCH, "-O1", "-g", "-std=c++17", "-ffp-contract=fast-honor-pragmas",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-x", "hip",
                           source, native.SRC_MPC_NOISE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "mpc noise host check ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------- the numpy statements
def test_colored_deviate_with_beta_zero_is_the_base_deviate_word_for_word():
    tick = np.array([0, 5, (1 << 32) + 3], dtype=np.int64)
    z = mpc.noise_deviate(77, 3, 50, tick, 12)
    eps = mpc_noise.colored_deviate(77, 3, 50, tick, 12, 0.0)
    assert np.array_equal(bits(eps), bits(z))
    assert not eps[:, 0].any()
    # a correlated table keeps sample 0 at zero and step 0 at the base deviate's words, and differs behind it
    col = mpc_noise.colored_deviate(77, 3, 50, tick, 12, [0.8, 0.0])
    assert not col[:, 0].any() and np.array_equal(bits(col[:, :, 0]), bits(z[:, :, 0]))
    assert np.array_equal(bits(col[..., 1]), bits(z[..., 1])) and not np.array_equal(bits(col[:, :, 1:, 0]), bits(z[:, :, 1:, 0]))
    b, g = mpc_noise.gains([0.8, 0.0])
    assert b.dtype == g.dtype == f32 and g[1] == 1.0 and g[0] == f32(np.sqrt(1.0 - np.float64(f32(0.8)) ** 2))
    k = 4
    want = (b[0] * col[1, 7, k - 1, 0]).astype(f32) + (g[0] * z[1, 7, k, 0]).astype(f32)
    assert bits(col[1, 7, k, 0]) == bits(want)
    assert mpc_noise.table_layout(col).shape == (12, 150, 2)
    assert np.array_equal(mpc_noise.table_layout(col)[k, 57], col[1, 7, k])


def test_statistics_of_the_colored_deviate():
    """Seed 77, tick 5, one plant, K = 65536, H = 12, BETA 0.8: per (k, a) the variance of eps * K0 within 0.02 of 1 and the
    correlation of successive steps within 0.02 of 0.8; 0.02 = 5 / sqrt(65536)."""
    K, H, beta = 65536, 12, 0.8
    bound = 5.0 / np.sqrt(K)
    assert abs(bound - 0.02) < 5e-4
    eps = mpc_noise.colored_deviate(77, 1, K, 5, H, beta)[0, 1:].astype(np.float64) * K0       # (sample 0 is the nominal)
    var = eps.var(axis=0)
    print("variance per (k, a): %.4f .. %.4f" % (var.min(), var.max()))
    assert var.shape == (H, 2) and np.abs(var - 1.0).max() <= 0.02
    corr = np.array([[np.corrcoef(eps[:, k, a], eps[:, k + 1, a])[0, 1] for a in range(2)] for k in range(H - 1)])
    print("lag-1 correlation per (k, a): %.4f .. %.4f" % (corr.min(), corr.max()))
    assert np.abs(corr - beta).max() <= 0.02
    across = np.corrcoef(eps[:, 3, 0], eps[:, 3, 1])[0, 1]                                      # the components stay independent
    assert abs(across) <= 0.02


def _hand(M, K, H, value):
    """A hand-made table: eps * K0 = ``value`` [M, K, H, 2] exactly enough (float32 of value / K0)."""
    return (np.broadcast_to(np.asarray(value, dtype=np.float64), (M, K, H, 2)) / K0).astype(f32)


ADAPT = {"RATE": 0.25, "SIGMA_MIN": [0.05, 0.05], "SIGMA_MAX": [1.0, 1.0]}


def test_noise_replay_on_hand_made_costs():
    M, K, H, clip = 1, 4, 3, 1.0
    nominal = np.zeros((M, H, 2), f32)
    # sample j perturbs by j * 0.1 on the rail and by j * 0.05 on the pressure, at every step; sigma 0.5
    value = np.zeros((M, K, H, 2))
    value[0, :, :, 0] = (np.arange(K) * 0.1 / 0.5)[:, None]
    value[0, :, :, 1] = (np.arange(K) * 0.05 / 0.5)[:, None]
    eps = _hand(M, K, H, value)
    u = mpc_noise.colored_actions(nominal, [0.5, 0.5], eps, clip)
    assert np.allclose(u[0, :, 0, 0], np.arange(K) * 0.1, atol=1e-7) and np.allclose(u[0, :, 2, 1], np.arange(K) * 0.05, atol=1e-7)
    # equal costs: v is the plain mean square of d: (0 + 0.01 + 0.04 + 0.09) / 4 = 0.035, and a quarter of it on the pressure
    r = mpc_noise.noise_replay(nominal, np.zeros(K), 0.5, 0.05, 0, 0, clip, 0.0, adapt=ADAPT, eps=eps)
    assert np.allclose(r["v"][0], [0.035, 0.00875], rtol=1e-6) and np.allclose(r["weights"], 1.0)
    want = np.sqrt(0.75 * 0.25 + 0.25 * np.array([0.035, 0.00875]))
    assert np.allclose(r["sigma"][0], want, rtol=1e-6) and r["sigma"].dtype == f32
    assert np.allclose(r["new"][0, :, 0], 0.15, atol=1e-7)                 # ... and the new nominal is the plain mean
    # one dominating sample: v is that sample's mean square
    cost = np.array([50.0, 50.0, 0.0, 50.0])
    r = mpc_noise.noise_replay(nominal, cost, 0.5, 0.05, 0, 0, clip, 0.0, adapt=ADAPT, eps=eps)
    assert np.allclose(r["v"][0], [0.04, 0.01], rtol=1e-6) and np.allclose(r["new"][0, :, 0], 0.2, atol=1e-7)
    # the floor: every perturbation zero and the old sigma small; the ceiling: large perturbations
    tight = dict(ADAPT, RATE=1.0)
    r = mpc_noise.noise_replay(nominal, np.zeros(K), 0.5, 0.05, 0, 0, clip, 0.0, adapt=tight, eps=np.zeros_like(eps))
    assert np.array_equal(r["sigma"], np.full((1, 2), 0.05, f32)) and not r["v"].any()
    r = mpc_noise.noise_replay(nominal, np.zeros(K), 0.5, 0.05, 0, 0, 100.0, 0.0, adapt=tight, eps=_hand(M, K, H, 8.0))
    assert np.array_equal(r["sigma"], np.ones((1, 2), f32)) and np.allclose(r["v"], 16.0, rtol=1e-6)
    # d is taken after the clamp: the same table under clip 1 cannot spread further than the clamp lets it
    r = mpc_noise.noise_replay(nominal, np.zeros(K), 0.5, 0.05, 0, 0, 1.0, 0.0, adapt=dict(tight, SIGMA_MAX=[9.0, 9.0]),
                               eps=_hand(M, K, H, 8.0))
    assert np.allclose(r["v"], 1.0) and np.allclose(r["sigma"], 1.0)
    # the amplitude in force is sigma_p, not the configuration's
    r = mpc_noise.noise_replay(nominal, np.zeros(K), 0.5, 0.05, 0, 0, clip, 0.0, sigma_p=[[0.25, 1.0]], adapt=ADAPT, eps=eps)
    assert np.allclose(r["v"][0], [0.035 / 4, 0.00875 * 4], rtol=1e-6)
    assert np.allclose(r["sigma"][0], np.sqrt(0.75 * np.array([0.0625, 1.0]) + 0.25 * r["v"][0]), rtol=1e-6)


def test_noise_replay_branches_leave_or_reset_sigma():
    M, K, H, clip = 3, 5, 4, 1.0
    rng = np.random.default_rng(3)
    nominal = rng.uniform(-0.5, 0.5, (M, H, 2)).astype(f32)
    sigma_p = np.array([[0.3, 0.2], [0.7, 0.6], [0.15, 0.9]], f32)
    cost = rng.uniform(0, 0.5, (M, K))
    cost[1] = np.inf                                                        # no finite cost
    reset = np.array([0, 0, 1])                                             # plant 2's reset is consumed
    tick = np.array([3, 4, 5])
    r = mpc_noise.noise_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, [0.8, 0.5], sigma_p=sigma_p, adapt=ADAPT,
                               plant_reset=reset)
    assert not np.array_equal(bits(r["sigma"][0]), bits(sigma_p[0])) and np.isfinite(r["v"][0]).all()
    assert np.array_equal(bits(r["sigma"][1]), bits(sigma_p[1])) and np.isnan(r["v"][1]).all()
    assert np.array_equal(r["sigma"][2], np.array([0.5, 0.25], f32))
    assert np.array_equal(r["nominal"][1, :-1], nominal[1, 1:]) and not r["nominal"][2].any() and not r["plant_actions"][2].any()
    # a reset wins over "no finite cost"
    r2 = mpc_noise.noise_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, [0.8, 0.5], sigma_p=sigma_p, adapt=ADAPT,
                                plant_reset=np.array([0, 1, 0]))
    assert np.array_equal(r2["sigma"][1], np.array([0.5, 0.25], f32))
    # ADAPT off: sigma is left alone everywhere, and everything else is what ADAPT on gives
    off = mpc_noise.noise_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, [0.8, 0.5], sigma_p=sigma_p,
                                 plant_reset=reset)
    assert np.array_equal(bits(off["sigma"]), bits(sigma_p))
    for key in ("u", "weights", "new", "nominal", "plant_actions", "history", "tick"):
        assert np.array_equal(off[key], r[key]), key
    assert np.array_equal(off["tick"], tick + 1)
    # BETA 0 and sigma_p = sigma: the base replay, word for word
    base = mpc.mpc_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, reset)
    same = mpc_noise.noise_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, 0.0, plant_reset=reset)
    for key in ("u", "weights", "new", "nominal", "plant_actions", "history"):
        a, b = np.asarray(base[key]), np.asarray(same[key])
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), key
