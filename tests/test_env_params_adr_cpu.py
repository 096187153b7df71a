"""ENV_PARAMS_ADR without a GPU: include/vine_env_adr.h against its ctypes mirror, every refusal of its host entry point
and of the configuration, utils/env_params.py adr_replay (its reduction to the redraw, widening and narrowing on hand-made
flags, the range formula), the episode log's join of a row to the range in force, and the file and checkpoint round trips.
Every comparison is bit for bit or on integers."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, load_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, episodes
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = {"DAMPING": [0.005, 0.1], "ACTION_DELAY": [0, 6], "LINK_MASS": [0.7, 1.4], "FPAM_K": [0.9, 1.1],
        "SMOOTHING_ALPHA_DEFLATE": {"values": [0.6, 0.75, 0.9]}}
NAMES = {"DAMPING": {"START": [0.02, 0.02], "STEP": 0.005}, "ACTION_DELAY": {"START": [1, 1], "STEP": 1},
         "LINK_MASS": {"START": [1.0, 1.0], "STEP": 0.05}}
SLOT = abi.ENV_REDRAW_NAMES.index


def env_cfg(names=NAMES, spec=SPEC, per_episode=True, **keys):
    return {"ENV_PARAMS": spec, "ENV_PARAMS_PER_EPISODE": per_episode, "ENV_PARAMS_ADR": dict({"NAMES": names}, **keys)}


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


@pytest.fixture()
def vcfg(lib):
    c = abi.VineConfig()
    assert lib.vine_config_default(C.byref(c)) == 0
    c.seed = 42
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_and_the_struct_size(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_env_adr.h")).read(), flags=re.S)
    for macro, value in (("ABI_VERSION", abi.ENV_ADR_ABI_VERSION), ("THREADS", abi.ENV_ADR_THREADS),
                         ("HISTORY_WORDS", abi.ENV_ADR_HISTORY_WORDS), ("KEY_PROBE", abi.ENV_ADR_KEY_PROBE),
                         ("KEY_WHICH", abi.ENV_ADR_KEY_WHICH)):
        assert int(re.search(r"#define VINE_ENV_ADR_%s (\w+?)(ull)?\s" % macro, text).group(1), 0) == value, macro
    for word, key in (("ADR_PROBE", abi.ENV_ADR_KEY_PROBE), ("ADR_WHICH", abi.ENV_ADR_KEY_WHICH)):
        assert key == env_params.name_key(word) == int.from_bytes(hashlib.sha256(word.encode()).digest()[:8], "little")
    for struct, mirror in (("VineEnvAdrName", abi.VineEnvAdrName), ("VineEnvAdrSpec", abi.VineEnvAdrSpec)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        fields = [f for decl in body.split(";") if decl.strip()
                  for f in re.sub(r"\[.*?\]", "", decl.strip().split(None, 1)[-1]).replace(" ", "").split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(abi.VineEnvAdrName) == 32
    assert lib.vine_env_adr_spec_size() == C.sizeof(abi.VineEnvAdrSpec) == 712 + C.sizeof(abi.VineEnvRedrawSpec) == 1632
    assert abi.VineEnvAdrSpec.redraw.offset == 712
    functions = sorted(set(re.findall(r"\b(vine_env_adr[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.ENV_ADR_PROTOTYPES)
    for name in functions:
        assert hasattr(lib, name), name
    # the eighth translation unit; it forms columns, so it is compiled without contraction: by its own pragma, which the
    # flag makes the compiler honour
    assert native.SOURCES[7] == native.SRC_ADR and len(native.SOURCES) == 8
    assert any(d.endswith("vine_env_adr.h") for d in native.DEPS) and any(d.endswith("vine_env_redraw_draw.h") for d in native.DEPS)
    flags = native._flags(native.SRC_ADR)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast")      # (the later one wins)
    source = open(native.SRC_ADR).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    csrc = os.path.dirname(native.SRC_ADR)
    draw = open(os.path.join(csrc, "vine_env_redraw_draw.h")).read()
    assert '#include "vine_named_draw.h"' in draw and any(d.endswith("vine_named_draw.h") for d in native.DEPS)
    draw += open(os.path.join(csrc, "vine_named_draw.h")).read()      # (the named draw itself: what the column header includes)
    for function in ("mix64", "redraw_u", "redraw_value", "redraw_column", "names_inertia"):      # stated once, in the headers
        assert len(re.findall(r"inline \w[\w ]* %s\(" % function, draw)) == 1, function
        assert not re.search(r"inline \w[\w ]* %s\(" % function, open(native.SRC_REDRAW).read()), function


def _adr_call(lib, vcfg, names=None, spec=SPEC, fraction=0.25, queue=4, widen_at=0.8, narrow_at=0.4, capacity=16, redraw=None,
              cfg=True, out=True):
    rspec = env_params.redraw_spec(lib, vcfg, spec, 0x1000) if redraw is None else redraw
    names = env_params.adr_names({"NAMES": NAMES}) if names is None else names
    a = abi.VineEnvAdrSpec()
    rc = lib.vine_env_adr_spec(C.byref(vcfg) if cfg else None, C.byref(rspec) if rspec is not False else None, names, fraction,
                               queue, widen_at, narrow_at, capacity, C.byref(a) if out else None)
    return rc, lib.vine_last_error().decode(), a


def test_the_spec_and_every_refusal_by_name(lib, vcfg):
    rc, _, a = _adr_call(lib, vcfg)
    assert rc == abi.OK and a.checked == 1 and a.redraw.checked == 1 and a.num_adr == 3 and a.queue == 4 and a.history_capacity == 16
    assert (a.boundary_fraction, a.widen_at, a.narrow_at) == (0.25, 0.8, 0.4)
    assert list(a.adr_slot)[:3] == [SLOT("DAMPING"), SLOT("ACTION_DELAY"), SLOT("LINK_MASS")] and set(list(a.adr_slot)[3:]) == {-1}
    want = env_params.adr_max_widen(SPEC, {"NAMES": NAMES})
    assert np.array_equal(np.array([list(r) for r in a.max_widen]), want)
    assert want[SLOT("ACTION_DELAY")].tolist() == [1, 5] and want[SLOT("FPAM_K")].tolist() == [0, 0]
    assert a.redraw.name[SLOT("DAMPING")].lo == 0.005 and a.name[SLOT("DAMPING")].start_lo == 0.02 and a.name[SLOT("FPAM_K")].on == 0
    # null pointers, an unchecked redraw spec
    assert _adr_call(lib, vcfg, cfg=False)[:2] == (abi.ERR_INVALID_ARG, "null argument to vine_env_adr_spec")
    assert _adr_call(lib, vcfg, out=False)[0] == abi.ERR_INVALID_ARG and _adr_call(lib, vcfg, redraw=False)[0] == abi.ERR_INVALID_ARG
    unchecked = env_params.redraw_spec(lib, vcfg, SPEC, 0x1000)
    unchecked.checked = 0
    rc, msg, _ = _adr_call(lib, vcfg, redraw=unchecked)
    assert rc == abi.ERR_INVALID_ARG and "was not filled by vine_env_redraw_spec" in msg
    # the scalars
    for kw, match in ((dict(fraction=1.0), "BOUNDARY_FRACTION must lie in [0, 1)"), (dict(fraction=-0.1), "BOUNDARY_FRACTION"),
                      (dict(fraction=float("nan")), "BOUNDARY_FRACTION"), (dict(queue=0), "QUEUE must be at least 1"),
                      (dict(widen_at=0.4, narrow_at=0.4), "NARROW_AT must be below WIDEN_AT"),
                      (dict(widen_at=0.3, narrow_at=0.5), "NARROW_AT must be below WIDEN_AT"),
                      (dict(capacity=0), "history capacity must be at least 1")):
        rc, msg, _ = _adr_call(lib, vcfg, **kw)
        assert rc == abi.ERR_INVALID_ARG and match in msg, (kw, msg)
    # the names
    def one(name="DAMPING", **kw):
        n = (abi.VineEnvAdrName * abi.VR_NAMES)()
        nm = n[SLOT(name)]
        nm.on, nm.start_lo, nm.start_hi, nm.step = 1, NAMES.get(name, NAMES["DAMPING"])["START"][0], \
            NAMES.get(name, NAMES["DAMPING"])["START"][1], NAMES.get(name, NAMES["DAMPING"])["STEP"]
        for k, v in kw.items():
            setattr(nm, k, v)
        return n
    assert _adr_call(lib, vcfg, one())[0] == abi.OK
    for names, match in ((one(start_lo=0.004), "DAMPING: START lies outside the limits"), (one(start_hi=0.2), "START lies outside"),
                         (one(start_lo=0.03), "DAMPING: START needs finite lo <= hi"), (one(start_hi=float("nan")), "START needs finite"),
                         (one(step=0.0), "DAMPING: STEP must be positive"), (one(step=-1.0), "STEP must be positive"),
                         (one(step=float("inf")), "STEP must be positive"), (one(reserved=1), "reserved must be 0"),
                         (one(step=1e-12), "more than 2^30 STEPs"),
                         (one("ACTION_DELAY", start_lo=0.5), "ACTION_DELAY: an integer parameter takes an integer START and STEP"),
                         (one("ACTION_DELAY", step=0.5), "ACTION_DELAY: an integer parameter takes an integer START and STEP"),
                         (one("SMOOTHING_ALPHA_DEFLATE"), "SMOOTHING_ALPHA_DEFLATE: a name under ADR must be a [lo, hi] range"),
                         (one("RAIL_P_GAIN"), "RAIL_P_GAIN: a name under ADR must be a [lo, hi] range"),
                         ((abi.VineEnvAdrName * abi.VR_NAMES)(), "no name is under ADR")):
        rc, msg, _ = _adr_call(lib, vcfg, names)
        assert rc == abi.ERR_INVALID_ARG and match in msg, msg
    off = (abi.VineEnvAdrName * abi.VR_NAMES)()
    off[0].on, off[0].start_lo, off[0].start_hi, off[0].step = 1, 0.02, 0.02, 0.005
    off[3].step = 1.0
    rc, msg, _ = _adr_call(lib, vcfg, off)
    assert rc == abi.ERR_INVALID_ARG and "RAIL_VELOCITY_SCALE: START and STEP of a name that is not under ADR must be 0" in msg
    # the python wrapper raises with the library's text
    with pytest.raises(ValueError, match="ENV_PARAMS_ADR: env adr spec: QUEUE must be at least 1"):
        env_params.adr_spec(lib, vcfg, SPEC, dict(env_params.adr_config(env_cfg()), QUEUE=0), 0x1000)
    # the launch refuses what it can without a device: nulls, a spec nobody checked
    args = [None, C.byref(a)] + [8] * 10 + [None]
    assert lib.vine_env_adr_scheduled(*args) == abi.ERR_INVALID_ARG and b"null argument to vine_env_adr_scheduled" in lib.vine_last_error()


def test_packaged_default_and_every_config_error():
    env = load_config()["task"]["env"]
    assert env["ENV_PARAMS_ADR"] == {} and env_params.adr_config(env) is None
    assert env_params.adr_config({"ENV_PARAMS_ADR": {}, "ENV_PARAMS": SPEC}) is None
    adr = env_params.adr_config(env_cfg(QUEUE=4))
    assert list(adr["NAMES"]) == ["DAMPING", "ACTION_DELAY", "LINK_MASS"] and adr["QUEUE"] == 4 and adr["HISTORY_CAPACITY"] == 1024
    assert (adr["BOUNDARY_FRACTION"], adr["WIDEN_AT"], adr["NARROW_AT"]) == (0.25, 0.8, 0.4)
    assert adr["NAMES"]["ACTION_DELAY"] == {"START": [1.0, 1.0], "STEP": 1.0}

    def names(name, **kw):
        return dict(NAMES, **{name: dict(NAMES.get(name, NAMES["DAMPING"]), **kw)})
    for cfg, kw, match in (
            (env_cfg(per_episode=False), {}, "ENV_PARAMS_ADR needs task.env.ENV_PARAMS_PER_EPISODE"),
            (env_cfg(), dict(multi_gpu=True), "ENV_PARAMS_ADR with multi_gpu=True"),
            (env_cfg(names("FPAM_C")), {}, r"ENV_PARAMS_ADR\.NAMES\.FPAM_C: the name must be a \[lo, hi\] range"),
            (env_cfg(names("SMOOTHING_ALPHA_DEFLATE")), {}, r"NAMES\.SMOOTHING_ALPHA_DEFLATE: the name must be a \[lo, hi\] range"),
            (env_cfg(names("NO_SUCH")), {}, r"NAMES\.NO_SUCH: unknown parameter"),
            (env_cfg({}), {}, r"ENV_PARAMS_ADR\.NAMES must map at least one name"),
            (env_cfg(names("DAMPING", START=[0.001, 0.02])), {}, r"NAMES\.DAMPING\.START \[0\.001, 0\.02\] lies outside the limits"),
            (env_cfg(names("DAMPING", START=[0.02, 0.2])), {}, r"NAMES\.DAMPING\.START .* lies outside the limits"),
            (env_cfg(names("DAMPING", START=[0.03, 0.02])), {}, r"NAMES\.DAMPING\.START: lo > hi"),
            (env_cfg(names("DAMPING", START=[0.02])), {}, r"NAMES\.DAMPING\.START is \[lo, hi\]"),
            (env_cfg(names("DAMPING", STEP=0)), {}, r"NAMES\.DAMPING\.STEP must be positive"),
            (env_cfg(names("DAMPING", STEP=-0.01)), {}, r"NAMES\.DAMPING\.STEP must be positive"),
            (env_cfg(names("DAMPING", STEP="x")), {}, r"NAMES\.DAMPING\.STEP: 'x' is not a number"),
            (env_cfg(names("ACTION_DELAY", START=[0.5, 1])), {}, r"NAMES\.ACTION_DELAY: an integer parameter takes an integer START and STEP"),
            (env_cfg(names("ACTION_DELAY", STEP=1.5)), {}, r"NAMES\.ACTION_DELAY: an integer parameter takes an integer START and STEP"),
            (env_cfg(WIDEN_AT=0.4, NARROW_AT=0.4), {}, r"ENV_PARAMS_ADR\.NARROW_AT \(0\.4\) must be below WIDEN_AT"),
            (env_cfg(NARROW_AT=0.9), {}, r"NARROW_AT \(0\.9\) must be below WIDEN_AT"),
            (env_cfg(BOUNDARY_FRACTION=1.0), {}, r"ENV_PARAMS_ADR\.BOUNDARY_FRACTION must lie in \[0, 1\)"),
            (env_cfg(BOUNDARY_FRACTION=-0.5), {}, r"BOUNDARY_FRACTION must lie in \[0, 1\)"),
            (env_cfg(QUEUE=0), {}, r"ENV_PARAMS_ADR\.QUEUE must be an integer >= 1"),
            (env_cfg(QUEUE=2.5), {}, r"QUEUE must be an integer >= 1"),
            (env_cfg(HISTORY_CAPACITY=0), {}, r"HISTORY_CAPACITY must be an integer >= 1"),
            (env_cfg(SPEED=3), {}, r"ENV_PARAMS_ADR: unknown key\(s\) SPEED")):
        with pytest.raises(ConfigError, match=match):
            env_params.adr_config(cfg, **kw)


def test_candidate_config_and_the_test_entry_switch_it_off_and_log(caplog, monkeypatch, tmp_path):
    import logging
    from vine_robot_isaacgymenvs_amd import train
    from vine_robot_isaacgymenvs_amd.learning import a2c_continuous
    from vine_robot_isaacgymenvs_amd.utils import sysid
    assert ("env", "ENV_PARAMS_ADR", {}) in sysid.FORCED
    cfg = load_config()["task"]
    cfg["env"].update(env_cfg())
    with caplog.at_level(logging.INFO):
        out = sysid.candidate_config(cfg, {"DAMPING": [0.01, 0.05]}, 70, 12)
    assert out["env"]["ENV_PARAMS_ADR"] == {} and out["env"]["ENV_PARAMS_PER_EPISODE"] is False
    assert any("ENV_PARAMS_ADR forced from" in r.getMessage() for r in caplog.records)
    # train.py's entry: test=True plays on the full limits, multi_gpu is refused before anything starts
    seen = {}
    monkeypatch.setattr(a2c_continuous.Runner, "run", lambda self, args: seen.update(args) or "ran")
    monkeypatch.chdir(tmp_path)
    over = ["task.env.ENV_PARAMS={DAMPING: [0.005, 0.1]}", "task.env.ENV_PARAMS_PER_EPISODE=True",
            "task.env.ENV_PARAMS_ADR={NAMES: {DAMPING: {START: [0.02, 0.02], STEP: 0.005}}}"]
    caplog.clear()
    cfg = load_config("config", overrides=over + ["test=True"])
    with caplog.at_level(logging.INFO):
        assert train.launch(cfg) == "ran"
    assert cfg["task"]["env"]["ENV_PARAMS_ADR"] == {} and seen["play"] is True
    assert any("ENV_PARAMS_ADR is forced off" in r.getMessage() for r in caplog.records)
    cfg = load_config("config", overrides=over + ["multi_gpu=True"])
    with pytest.raises(ConfigError, match="ENV_PARAMS_ADR with multi_gpu=True"):
        train.launch(cfg)


# ------------------------------------------------------------------------------------------------------------ the replay
def test_reduction_to_the_redraw(lib, vcfg):
    """BOUNDARY_FRACTION 0 and START = the limits: every (env, episode) column is draw_columns', bit for bit; nothing probes,
    nothing is counted, nothing moves."""
    spec = dict(SPEC, CART_MASS=[0.35, 0.7])
    names = {n: {"START": list(spec[n]), "STEP": s} for n, s in (("DAMPING", 0.01), ("ACTION_DELAY", 2), ("LINK_MASS", 0.1))}
    adr = env_params.adr_config(env_cfg(names, spec, BOUNDARY_FRACTION=0.0, QUEUE=1))
    gids = np.arange(1000, 1070)
    rng = np.random.default_rng(3)
    resets = rng.uniform(size=(30, 70)) < 0.3
    flags = rng.uniform(size=(30, 70)) < 0.5
    steps = env_params.adr_replay(spec, adr, 42, gids, resets, flags, vcfg, lib=lib)
    p0, i0 = env_params.build_columns(spec, vcfg, gids, 0, lib=lib)
    assert np.array_equal(resets.cumsum(0)[-1], steps[-1]["episode_index"])
    for t, s in enumerate(steps):
        p, i = env_params.build_columns(spec, vcfg, gids, resets[:t + 1].sum(0), lib=lib)
        assert np.array_equal(bits(s["params"]), bits(p)) and np.array_equal(bits(s["inertia"]), bits(i)), t
        assert (s["probe"] == -1).all() and not s["counts"].any() and not s["widen"].any() and s["cursor"] == 0
    assert not np.array_equal(bits(steps[-1]["params"]), bits(p0)) and i0 is not None


def scripted(lib, vcfg, reach, steps=60, n=64, queue=4, names=NAMES, fraction=0.9):
    """Every env resets at every step; every episode reaches iff reach(t)."""
    adr = env_params.adr_config(env_cfg(names, QUEUE=queue, BOUNDARY_FRACTION=fraction))
    resets = np.ones((steps, n), dtype=bool)
    flags = np.array([[bool(reach(t))] * n for t in range(steps)])
    return adr, env_params.adr_replay(SPEC, adr, 42, np.arange(n), resets, flags, vcfg, lib=lib)


def test_hand_made_flags_widen_narrow_and_stop(lib, vcfg):
    limit = env_params.adr_max_widen(SPEC, {"NAMES": NAMES})
    under = [SLOT(n) for n in NAMES]
    # all reached: every boundary widens by one per decision and stops at its limit
    adr, steps = scripted(lib, vcfg, lambda t: True)
    assert np.array_equal(steps[-1]["widen"][under], limit[under]) and limit[under].max() == 16
    h = steps[-1]["history"]
    assert len(h) == limit.sum() == steps[-1]["cursor"] and (h[:, 3] == 0).all() and (np.diff(h[:, 0]) >= 0).all()
    for b in np.unique(h[:, 1]):                                   # each boundary: 1, 2, ..., its limit, never beyond
        assert h[h[:, 1] == b, 2].tolist() == list(range(1, limit[b >> 1, b & 1] + 1))
    same_step = h[np.r_[False, np.diff(h[:, 0]) == 0]]             # rows of one step are in boundary order
    assert len(same_step) and all((np.diff(h[h[:, 0] == s, 1]) > 0).all() for s in np.unique(h[:, 0]))
    assert steps[0]["widen"].sum() == 0 and not steps[-1]["widen"][[SLOT("FPAM_K")]].any()
    ranges = env_params.adr_ranges(SPEC, adr, steps[-1]["widen"])
    assert ranges == {"DAMPING": (0.005, 0.1), "ACTION_DELAY": (0.0, 6.0), "LINK_MASS": (0.7, 1.4)}
    # an ADR run of ACTION_DELAY hits both integer ends of the range in force, and only integers
    delays = np.concatenate([s["params"][abi.VP_ACTION_DELAY] for s in steps[-10:]])
    assert delays.min() == 0 and delays.max() == 6 and np.array_equal(delays, np.floor(delays))
    assert steps[0]["params"][abi.VP_ACTION_DELAY].tolist() == [1.0] * 64          # (the first redraw: START is one point)
    # none reached: nothing ever leaves START, no history
    _, steps = scripted(lib, vcfg, lambda t: False)
    assert not steps[-1]["widen"].any() and steps[-1]["cursor"] == 0 and steps[-1]["counts"][under].sum() > 0
    # reached for 20 steps, then never: the boundaries come back one step per decision and stop at START
    _, steps = scripted(lib, vcfg, lambda t: t < 20, steps=150)
    assert steps[19]["widen"][under].min() >= 1
    assert not steps[-1]["widen"].any()
    h = steps[-1]["history"]
    for b in np.unique(h[:, 1]):
        w = h[h[:, 1] == b, 2]
        up = int(np.argmax(w))
        assert (np.diff(w[:up + 1]) == 1).all() and (np.diff(w[up:]) == -1).all() and w[-1] == 0 and w.min() >= 0
    # between NARROW_AT and WIDEN_AT nothing moves, and the counts are cleared all the same
    adr, steps = scripted(lib, vcfg, lambda t: t % 2 == 0, queue=1000, fraction=0.5)
    assert not steps[-1]["widen"].any() and steps[-1]["cursor"] == 0
    assert steps[-1]["counts"][under, :, 0].max() < 1000 + 64 and steps[-1]["counts"][under, :, 0].sum() < 64 * 60
    # a probing episode's value is exactly its boundary; the others lie inside the range in force
    adr, steps = scripted(lib, vcfg, lambda t: True, steps=12)
    for t in range(1, 12):
        s, ranges = steps[t], env_params.adr_ranges(SPEC, adr, steps[t]["widen"])
        d = s["params"][abi.VP_DAMPING]
        lo, hi = np.float32(ranges["DAMPING"][0]), np.float32(ranges["DAMPING"][1])
        assert (d[s["probe"] == 2 * SLOT("DAMPING")] == lo).all() and (d[s["probe"] == 2 * SLOT("DAMPING") + 1] == hi).all()
        assert (d >= lo).all() and (d <= hi).all()
        assert set(np.unique(s["probe"])) <= {-1} | {2 * SLOT(n) + side for n in NAMES for side in (0, 1)}
    assert len(set(np.concatenate([s["probe"] for s in steps]).tolist())) == 7


def test_the_range_formula_stays_inside_the_limits():
    rng = np.random.default_rng(5)
    for _ in range(200):
        lo, hi = np.sort(rng.uniform(-3.0, 3.0, 2))
        s_lo, s_hi = np.sort(rng.uniform(lo, hi, 2))
        step = float(rng.choice([1e-3, 0.05, 0.3, 7.0]))
        spec = {"DAMPING": [float(lo), float(hi)]}
        adr = {"NAMES": {"DAMPING": {"START": [float(s_lo), float(s_hi)], "STEP": step}}}
        top = env_params.adr_max_widen(spec, adr)[0]
        assert top.min() >= 0
        for w_lo in sorted({0, 1, int(top[0]) // 2, max(int(top[0]) - 1, 0), int(top[0])}):
            for w_hi in sorted({0, 1, int(top[1]) // 2, max(int(top[1]) - 1, 0), int(top[1])}):
                widen = np.zeros((abi.VR_NAMES, 2), dtype=np.int64)
                widen[0] = min(w_lo, top[0]), min(w_hi, top[1])
                a, b = env_params.adr_ranges(spec, adr, widen)["DAMPING"]
                assert lo <= a <= s_lo <= s_hi <= b <= hi
                if widen[0, 0] == top[0]:
                    assert a == lo
                if widen[0, 1] == top[1]:
                    assert b == hi


# ------------------------------------------------------------------------------------------------ the episode-log join
def test_rows_join_the_range_in_force_and_a_dropped_predecessor_gives_nan(lib, vcfg, tmp_path):
    """Two envs, every env resetting at steps 4, 9, 14, ... of a scripted all-reaching run with QUEUE 1, so the ranges move
    at almost every decision.  The log's rows (env, end step, episode) joined through the history give the replay's own
    column of that episode; with env 1's row of episode 2 dropped, its episode 3 has no known plant."""
    n, T = 2, 60
    adr = env_params.adr_config(env_cfg(QUEUE=1, BOUNDARY_FRACTION=0.6))
    resets = np.zeros((T, n), dtype=bool)
    resets[4::5] = True
    steps = env_params.adr_replay(SPEC, adr, 42, np.arange(n) + 7, resets, np.ones((T, n), dtype=bool), vcfg, lib=lib)
    history = steps[-1]["history"]
    assert len(history) >= 6
    env, end = np.nonzero(resets.T)
    episode = np.concatenate([np.arange(resets[:, e].sum()) for e in range(n)])
    at = episodes.drawn_at(env, episode, end)
    assert at[episode == 0].tolist() == [-1, -1] and np.array_equal(at[episode > 0], end[episode > 0] - 5)
    p, i, probe = env_params.adr_episode_columns(SPEC, adr, 42, env + 7, episode, at, history, vcfg=vcfg, lib=lib)
    for r in range(len(env)):                                      # the plant an episode RAN with: the table behind the step before
        want = steps[at[r]] if episode[r] else None                # its first step, i.e. behind the step that drew it
        if want is None:
            p0, i0 = env_params.build_columns(env_params.adr_start_spec(SPEC, adr), vcfg, [env[r] + 7], 0, lib=lib)
            assert np.array_equal(bits(p[:, r]), bits(p0[:, 0])) and np.array_equal(bits(i[:, r]), bits(i0[:, 0])) and probe[r] == -1
        else:
            assert np.array_equal(bits(p[:, r]), bits(want["params"][:, env[r]])), r
            assert np.array_equal(bits(i[:, r]), bits(want["inertia"][:, env[r]])) and probe[r] == want["probe"][env[r]]
    assert (probe >= 0).any() and len(np.unique(p[abi.VP_DAMPING])) > 4
    assert np.array_equal(env_params.adr_widen_at(history, [T - 1])[0], steps[-1]["widen"])
    assert not env_params.adr_widen_at(history, [history[0, 0] - 1]).any()
    # the same through the rows' dict, with a dropped predecessor
    rows = {name: np.zeros(len(env), dtype=np.int64 if name in episodes.INT_COLUMNS else np.float32) for name in episodes.COLUMNS}
    rows.update(env=env, end_step=end, episode=episode)
    columns = lambda e, k, a: env_params.adr_episode_columns(SPEC, adr, 42, np.asarray(e) + 7, k, a, history, vcfg=vcfg, lib=lib)  # noqa: E731
    out, unknown = episodes.with_adr_params(rows, columns)
    assert unknown == 0 and np.array_equal(out["probe"], probe) and np.array_equal(out["param_DAMPING"], p[abi.VP_DAMPING])
    assert np.array_equal(out["param_LINK_MASS"], i[abi.VI_LINK_MASS0]) and np.array_equal(out["param_ACTION_DELAY"], p[abi.VP_ACTION_DELAY])
    keep = ~((env == 1) & (episode == 2))
    kept = {k: v[keep] for k, v in rows.items()}
    out, unknown = episodes.with_adr_params(kept, columns)
    lost = (kept["env"] == 1) & (kept["episode"] == 3)
    assert unknown == 1 and lost.sum() == 1 and np.isnan(out["param_DAMPING"][lost]).all() and out["probe"][lost].tolist() == [-2]
    assert np.array_equal(out["param_DAMPING"][~lost], p[abi.VP_DAMPING][keep][~lost]) and np.array_equal(out["probe"][~lost], probe[keep][~lost])

    # the file: configuration and complete history ride along, and the offline reader rebuilds the same columns
    path = str(tmp_path / "e.npz")
    episodes.save(path, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {"maxEpisodeLength": 5},
                  redraw={"spec": SPEC, "seed": 42, "env_id_offset": 7, "base": env_params.config_row(lib, vcfg),
                          "inertia_base": env_params.inertia_config_row(lib, vcfg),
                          "geometry": (vcfg.link_length, vcfg.link_com, vcfg.gravity)},
                  adr={"config": adr, "history": history, "history_dropped": 0})
    config, stored, dropped, widen0, columns3 = episodes.load_env_adr(path)
    assert config == adr and np.array_equal(stored, history) and dropped == 0 and not widen0.any()
    p3, i3, probe3 = columns3(env, episode, at)
    assert np.array_equal(p3, p) and np.array_equal(i3, i) and np.array_equal(probe3, probe)
    stored_episode, columns2 = episodes.load_env_redraw(path)      # the section-20 reader keeps its signature and says where to go
    assert np.array_equal(stored_episode, episode)
    with pytest.raises(ValueError, match="written under ENV_PARAMS_ADR.*load_env_adr"):
        columns2(env, episode)
    back = episodes.load_rows_with_params(path)
    assert np.array_equal(back["probe"], probe) and np.array_equal(back["param_DAMPING"], p[abi.VP_DAMPING])
    assert np.array_equal(back["episode"], episode)
    plain = str(tmp_path / "plain.npz")
    episodes.save(plain, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {})
    assert episodes.load_env_adr(plain) == (None, None, 0, None, None) and "probe" not in episodes.load_rows_with_params(plain)


def stand_in(adr):
    """An ``EnvAdr`` that holds host tensors: what ``state_dict`` / ``load_state_dict`` and the join touch."""
    import torch
    from vine_robot_isaacgymenvs_amd.utils import env_adr
    a = env_adr.EnvAdr.__new__(env_adr.EnvAdr)
    a.spec, a.adr, a.widen = SPEC, adr, torch.zeros((abi.VR_NAMES, 2), dtype=torch.int32)
    a.widen0, a.cursor, a.history_harvested = np.zeros((abi.VR_NAMES, 2), dtype=np.int64), torch.zeros(1, dtype=torch.int64), 0
    a.history_rows = np.zeros((0, 4), dtype=np.int64)
    return a


def test_the_checkpoint_entry_round_trip():
    """``EnvAdr.state_dict`` / ``load_state_dict`` on a stand-in: what the checkpoint keeps is ``widen``; a widen that does
    not fit the configuration is refused, and so is a restore into a run under way."""
    import torch
    adr = env_params.adr_config(env_cfg())
    a = stand_in(adr)
    a.widen[SLOT("DAMPING"), 1], a.widen[SLOT("ACTION_DELAY"), 0] = 5, 1
    state = a.state_dict()
    assert state["names"] == list(NAMES) and state["widen"][SLOT("DAMPING")].tolist() == [0, 5]
    b = stand_in(adr)
    b.load_state_dict(state)
    assert torch.equal(a.widen, b.widen) and np.array_equal(b.widen0, state["widen"])
    state["widen"][SLOT("ACTION_DELAY"), 0] = 2                    # beyond the limit: one step from START 1 to 0
    with pytest.raises(ValueError, match="does not fit this configuration"):
        b.load_state_dict(state)
    with pytest.raises(ValueError, match="does not fit"):
        b.load_state_dict({"widen": a.state_dict()["widen"], "names": ["DAMPING"]})
    b.cursor[0] = 3
    with pytest.raises(RuntimeError, match="before the first step"):
        b.load_state_dict(a.state_dict())


def test_a_resumed_run_joins_its_rows_to_the_restored_ranges(lib, vcfg, tmp_path):
    """A run resumed from a checkpoint whose widen is not zero: ``load_state_dict`` keeps it as ``widen0``, the replay starts
    from it, and the join -- the observer's and the file's -- gives the replay's own column of every episode.  The history of
    the resumed run holds no row for what the checkpoint brought; a join that began at zero would draw episode 1 from START."""
    n, T = 24, 40
    adr = env_params.adr_config(env_cfg(QUEUE=2, BOUNDARY_FRACTION=0.5))
    first = stand_in(adr)
    first.widen[SLOT("DAMPING"), 0], first.widen[SLOT("DAMPING"), 1] = 2, 7
    first.widen[SLOT("LINK_MASS"), 1], first.widen[SLOT("ACTION_DELAY"), 1] = 4, 3
    resumed = stand_in(adr)
    resumed.load_state_dict(first.state_dict())
    widen0 = resumed.widen0
    assert widen0.sum() == 16 and widen0[SLOT("DAMPING")].tolist() == [2, 7]
    resets = np.zeros((T, n), dtype=bool)
    resets[3::4] = True
    reach = np.ones((T, n), dtype=bool)
    reach[20:] = False                                             # widening first, narrowing later: rows on both sides of widen0
    steps = env_params.adr_replay(SPEC, adr, 42, np.arange(n), resets, reach, vcfg, lib=lib, widen0=widen0)
    assert np.array_equal(steps[0]["widen"], widen0) and len(steps[-1]["history"]) >= 4
    assert np.array_equal(env_params.adr_widen_at(steps[-1]["history"], [-1, T - 1], widen0), [widen0, steps[-1]["widen"]])
    env, end = np.nonzero(resets.T)
    episode = np.concatenate([np.arange(resets[:, e].sum()) for e in range(n)])
    at = episodes.drawn_at(env, episode, end)
    resumed.history_rows, resumed.seed, resumed.env_id_offset, resumed.vcfg, resumed.lib = steps[-1]["history"], 42, 0, vcfg, lib
    p, i, probe = resumed.episode_columns(env, episode, at)
    wrong = env_params.adr_episode_columns(SPEC, adr, 42, env, episode, at, steps[-1]["history"], vcfg=vcfg, lib=lib)[0]
    later = np.flatnonzero(episode > 0)
    for r in later:
        want = steps[at[r]]
        assert np.array_equal(bits(p[:, r]), bits(want["params"][:, env[r]])) and probe[r] == want["probe"][env[r]], r
        assert np.array_equal(bits(i[:, r]), bits(want["inertia"][:, env[r]])), r
    assert not np.array_equal(p[:, later], wrong[:, later])       # (what a join from zero gives is not it)
    rows = {name: np.zeros(len(env), dtype=np.int64 if name in episodes.INT_COLUMNS else np.float32) for name in episodes.COLUMNS}
    rows.update(env=env, end_step=end, episode=episode)
    path = str(tmp_path / "resumed.npz")
    episodes.save(path, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {},
                  redraw={"spec": SPEC, "seed": 42, "env_id_offset": 0, "base": env_params.config_row(lib, vcfg),
                          "inertia_base": env_params.inertia_config_row(lib, vcfg),
                          "geometry": (vcfg.link_length, vcfg.link_com, vcfg.gravity)},
                  adr={"config": adr, "history": steps[-1]["history"], "history_dropped": 0, "widen0": widen0})
    assert np.array_equal(episodes.load_env_adr(path)[3], widen0)
    back = episodes.load_rows_with_params(path)
    assert np.array_equal(back["probe"], probe) and np.array_equal(back["param_DAMPING"], p[abi.VP_DAMPING])


def test_the_launch_refuses_mismatched_specs_without_a_device(lib, vcfg):
    """The refusals of the two entry points that need no handle: an abi_version that is not this library's, in the redraw
    spec handed to vine_env_adr_spec and in the ADR spec (or the redraw spec inside it) handed to the launch; a spec nobody
    checked; value lists without their device array."""
    rspec = env_params.redraw_spec(lib, vcfg, SPEC, 0x1000)
    rspec.abi_version += 1
    rc, msg, _ = _adr_call(lib, vcfg, redraw=rspec)
    assert rc == abi.ERR_INVALID_ARG and "VineEnvRedrawSpec.abi_version mismatch" in msg
    good = env_params.adr_spec(lib, vcfg, SPEC, env_params.adr_config(env_cfg()), 0x1000)

    def launch(**fields):
        a = abi.VineEnvAdrSpec.from_buffer_copy(good)
        for k, v in fields.items():
            target, _, field = k.rpartition("__")
            setattr(getattr(a, target) if target else a, field, v)
        rc = lib.vine_env_adr_scheduled(*([8, C.byref(a)] + [8] * 10 + [None]))
        return rc, lib.vine_last_error().decode()
    for fields, match in ((dict(abi_version=good.abi_version + 1), "VineEnvAdrSpec.abi_version mismatch"),
                          (dict(checked=0), "not filled by vine_env_adr_spec"), (dict(redraw__checked=0), "not filled by vine_env_adr_spec"),
                          (dict(redraw__abi_version=good.redraw.abi_version + 1), "VineEnvRedrawSpec.abi_version mismatch"),
                          (dict(redraw__values=None), "VineEnvRedrawSpec.values is NULL")):
        rc, msg = launch(**fields)
        assert rc == abi.ERR_INVALID_ARG and match in msg, (fields, msg)


def test_the_device_code_holds_no_contracted_multiply_add(tmp_path):
    """vine_env_adr.hip relies on a pragma for what vine_env_redraw.hip gets from its flag.  Compiled for the device with
    native.py's flags, every float64 fused multiply-add left in its assembly must be the exact one of a conversion to a
    64-bit integer, x - floor(x * 2^-32) * 2^32 (the literal 0xc1f00000 is -2^32's high word); a contracted `a + b * c` of
    the source would be one without it.  The same compile with the pragma defined away must show such contractions, so the
    check can fail."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def fused(name, extra):
        out = str(tmp_path / name)
        subprocess.check_call([hipcc] + native._flags(native.SRC_ADR) + extra + ["--cuda-device-only", "-S", "-o", out, native.SRC_ADR],
                              stderr=subprocess.DEVNULL)
        lines = [ln for ln in open(out) if re.search(r"\bv_fma(c|ak|mk)?_f64", ln)]
        return len(lines), [ln.strip() for ln in lines if "0xc1f00000" not in ln]
    total, contracted = fused("adr.s", [])
    assert total > 0 and contracted == [], contracted[:3]
    _, contracted = fused("adr_fast.s", ["-ffp-contract=fast"])    # (the later flag wins: the pragma is ignored again)
    assert len(contracted) > 10
