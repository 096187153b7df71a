"""ENV_PARAMS_PER_EPISODE without a GPU: include/vine_env_redraw.h against its ctypes mirror, the refusals of its host entry
point, the per-episode draw of utils/env_params.py (episode 0 = today's tables, shards, ends, checks, statistics), and the
episode log's join of a row to its episode's plant."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import env_inertia_sets, env_params_sets
from vine_robot_isaacgymenvs_amd import abi, load_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, episodes
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = {"DAMPING": [0.01, 0.05], "SMOOTHING_ALPHA_INFLATE": [0.6, 0.95], "SMOOTHING_ALPHA_DEFLATE": {"values": [0.6, 0.75, 0.9]},
        "RAIL_VELOCITY_SCALE": [0.7, 1.3], "RAIL_P_GAIN": 9.0, "RAIL_D_GAIN": [0.0, 0.4], "RAIL_ACCELERATION": [5.6, 10.4],
        "ACTION_DELAY": [0, 8], "FPAM_K": [0.8, 1.2], "FPAM_C": [0.8, 1.2], "FPAM_b": {"values": [0.9, 1.1]}, "FPAM_B": [0.8, 1.2],
        "CART_MASS": [0.35, 0.7], "LINK_MASS": [0.8, 1.3], "TIP_LINK_MASS": {"values": [1.0, 1.5, 2.0]}}


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
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_env_redraw.h")).read(), flags=re.S)

    def enum(name):
        body = re.search(r"typedef enum %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        value, out = -1, {}
        for item in [i.strip() for i in body.split(",") if i.strip()]:
            key, _, v = [x.strip() for x in item.partition("=")]
            value = int(v) if v else value + 1
            out[key] = value
        return out
    slots = enum("VineEnvRedrawSlot")
    assert slots.pop("VR_NAMES") == abi.VR_NAMES == len(abi.ENV_REDRAW_NAMES) == 15
    assert [k[3:] for k, _ in sorted(slots.items(), key=lambda kv: kv[1])] == list(abi.ENV_REDRAW_NAMES)
    assert abi.ENV_REDRAW_NAMES == abi.ENV_PARAM_NAMES + abi.ENV_INERTIA_NAMES
    assert enum("VineEnvRedrawForm") == {"VINE_REDRAW_ABSENT": abi.REDRAW_ABSENT, "VINE_REDRAW_NUMBER": abi.REDRAW_NUMBER,
                                         "VINE_REDRAW_RANGE": abi.REDRAW_RANGE, "VINE_REDRAW_VALUES": abi.REDRAW_VALUES}
    assert int(re.search(r"#define VINE_ENV_REDRAW_ABI_VERSION (\d+)", text).group(1)) == abi.ENV_REDRAW_ABI_VERSION
    assert int(re.search(r"#define VINE_ENV_REDRAW_THREADS (\d+)", text).group(1)) == abi.ENV_REDRAW_THREADS == 256
    for struct, mirror in (("VineEnvRedrawName", abi.VineEnvRedrawName), ("VineEnvRedrawSpec", abi.VineEnvRedrawSpec)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        fields = [f for decl in body.split(";") if decl.strip()
                  for f in re.sub(r"\[.*?\]", "", decl.strip().split(None, 2 if decl.strip().startswith("const") else 1)[-1]
                                  ).replace("*", "").replace(" ", "").split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert lib.vine_env_redraw_spec_size() == C.sizeof(abi.VineEnvRedrawSpec) == 920 and C.sizeof(abi.VineEnvRedrawName) == 48
    functions = sorted(set(re.findall(r"\b(vine_env_redraw[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.ENV_REDRAW_PROTOTYPES)
    for name in functions:
        assert hasattr(lib, name), name
    assert any(d.endswith("vine_env_redraw.h") for d in native.DEPS) and native.SRC_REDRAW in native.SOURCES
    # the new translation unit, and only it, is compiled without contraction
    flags = native._flags(native.SRC_REDRAW)
    assert flags.index("-ffp-contract=off") > flags.index("-ffp-contract=fast")      # (the later one wins)
    for src in native.SOURCES:
        if src != native.SRC_REDRAW:
            assert "-ffp-contract=off" not in native._flags(src) and "-ffp-contract=fast" in native._flags(src)


def test_packaged_default_and_config_refusal():
    env = load_config()["task"]["env"]
    assert env["ENV_PARAMS_PER_EPISODE"] is False
    assert env_params.per_episode(env) is False
    assert env_params.per_episode({"ENV_PARAMS_PER_EPISODE": True, "ENV_PARAMS": {"DAMPING": [0.01, 0.02]}}) is True
    with pytest.raises(ConfigError, match="ENV_PARAMS_PER_EPISODE needs a non-empty"):
        env_params.per_episode({"ENV_PARAMS_PER_EPISODE": True, "ENV_PARAMS": {}})
    from vine_robot_isaacgymenvs_amd.utils import sysid
    assert ("env", "ENV_PARAMS_PER_EPISODE", False) in sysid.FORCED


def test_candidate_config_switches_it_off_and_logs(caplog):
    import logging
    from vine_robot_isaacgymenvs_amd.utils import sysid
    cfg = load_config()["task"]
    cfg["env"]["ENV_PARAMS_PER_EPISODE"] = True
    with caplog.at_level(logging.INFO):
        out = sysid.candidate_config(cfg, {"DAMPING": [0.01, 0.05]}, 70, 12)
    assert out["env"]["ENV_PARAMS_PER_EPISODE"] is False
    assert any("ENV_PARAMS_PER_EPISODE forced from True to False" in r.getMessage() for r in caplog.records)


def _spec_call(lib, vcfg, names, values=(), device=0x1000, out=True):
    v = np.asarray(values, dtype=np.float64)
    spec = abi.VineEnvRedrawSpec()
    rc = lib.vine_env_redraw_spec(C.byref(vcfg) if vcfg is not None else None, names, v.ctypes.data if len(v) else None,
                                  device if len(v) else None, len(v), C.byref(spec) if out else None)
    return rc, lib.vine_last_error().decode(), spec


def test_every_refusal_of_the_spec_is_reached_by_name(lib, vcfg):
    names, values = env_params.redraw_names(FULL)
    rc, _, spec = _spec_call(lib, vcfg, names, values)
    assert rc == abi.OK and spec.checked == 1 and spec.seed == 42 and spec.num_values == 8 and spec.values == 0x1000
    assert np.array_equal(bits(np.array(spec.base_params)), bits(env_params.config_row(lib, vcfg)))
    assert np.array_equal(bits(np.array(spec.base_inertia)), bits(env_params.inertia_config_row(lib, vcfg)[:abi.VI_PRIMARY_COUNT]))
    assert (spec.link_length, spec.link_com, spec.gravity) == (vcfg.link_length, vcfg.link_com, vcfg.gravity)
    slot = abi.ENV_REDRAW_NAMES.index
    assert spec.name[slot("TIP_LINK_MASS")].radix == 6 and spec.name[slot("FPAM_b")].radix == 3
    assert spec.name[slot("DAMPING")].key == env_params.name_key("DAMPING")
    # null pointers
    assert _spec_call(lib, None, names, values)[:2] == (abi.ERR_INVALID_ARG, "null argument to vine_env_redraw_spec")
    assert _spec_call(lib, vcfg, None, values)[0] == abi.ERR_INVALID_ARG
    assert _spec_call(lib, vcfg, names, values, out=False)[0] == abi.ERR_INVALID_ARG
    rc, msg, _ = _spec_call(lib, vcfg, names, values, device=None)
    assert rc == abi.ERR_INVALID_ARG and "value lists need a host and a device array" in msg
    # what vine_env_params_check / vine_env_inertia_check refuse, at an end of a range or in a list
    for bad, match in (({"SMOOTHING_ALPHA_INFLATE": [0.5, 1.5]}, "SMOOTHING_ALPHA_INFLATE of candidate 1 .* outside"),
                       ({"ACTION_DELAY": [0, 9]}, "ACTION_DELAY of candidate 1 .* not an integer in"),
                       ({"ACTION_DELAY": {"values": [0, 1.5]}}, "ACTION_DELAY of candidate 1 .* not an integer in"),
                       ({"RAIL_ACCELERATION": {"values": [8.0, 9.0, -1.0]}}, "RAIL_ACCELERATION of candidate 2 .* negative"),
                       ({"CART_MASS": [0.0, 0.5]}, "CART_MASS of candidate 0 .* a mass must be positive"),
                       ({"DAMPING": 0.02, "TIP_LINK_MASS": {"values": [1.0, -2.0]}}, r"LINK_MASS\[4\] of candidate 1 .* a mass must be positive")):
        with pytest.raises(ValueError, match=match):
            env_params.redraw_spec(lib, vcfg, bad, 0x1000)
    # malformed entries of the struct itself
    def one(**kw):
        n = (abi.VineEnvRedrawName * abi.VR_NAMES)()
        n[0].form, n[0].key, n[0].radix, n[0].lo, n[0].hi = abi.REDRAW_RANGE, 1, 1, 0.01, 0.05
        for k, v in kw.items():
            setattr(n[0], k, v)
        return n
    assert _spec_call(lib, vcfg, one())[0] == abi.OK
    for kw, match in ((dict(form=7), "DAMPING: unknown form"), (dict(lo=0.06), "DAMPING: a range needs finite lo <= hi"),
                      (dict(hi=float("inf")), "a range needs finite"), (dict(reserved=1), "reserved must be 0"),
                      (dict(form=abi.REDRAW_VALUES, values_first=0, values_count=3), "extent of the value list lies outside"),
                      (dict(form=abi.REDRAW_NUMBER, lo=float("nan")), "the number is not finite")):
        rc, msg, _ = _spec_call(lib, vcfg, one(**kw), [0.01, 0.02])
        assert rc == abi.ERR_INVALID_ARG and match in msg, (kw, msg)
    rc, msg, _ = _spec_call(lib, vcfg, (abi.VineEnvRedrawName * abi.VR_NAMES)())
    assert rc == abi.ERR_INVALID_ARG and "no name is present" in msg
    n = (abi.VineEnvRedrawName * abi.VR_NAMES)()
    n[7].form, n[7].lo, n[7].hi = abi.REDRAW_RANGE, 0.5, 3.0
    rc, msg, _ = _spec_call(lib, vcfg, n)
    assert rc == abi.ERR_INVALID_ARG and "ACTION_DELAY: an integer parameter takes an integer range" in msg
    # the launch refuses what it can without a device: nulls and a spec nobody checked
    assert lib.vine_env_redraw_scheduled(None, C.byref(spec), 8, 8, 8, 8, None) == abi.ERR_INVALID_ARG
    assert b"null argument to vine_env_redraw_scheduled" in lib.vine_last_error()


# ------------------------------------------------------------------------------------------------------------ the draw
def test_episode_zero_is_todays_hash_and_todays_tables(lib, vcfg):
    gids = np.arange(4096)
    for seed in (0, 42, 12345):
        for name in ("DAMPING", "ACTION_DELAY", "FPAM_K", "LINK_MASS"):
            assert np.array_equal(env_params.uniform01_episode(seed, name, gids, 0), env_params.uniform01(seed, name, gids))
    p, i = env_params.build_columns(FULL, vcfg, np.arange(300) + 5, 0, lib=lib)
    assert np.array_equal(bits(p), bits(env_params.build_table(FULL, vcfg, 42, 300, 5, lib=lib)))
    assert np.array_equal(bits(i), bits(env_params.build_inertia_table(FULL, vcfg, 42, 300, 5, lib=lib)))
    # the nine parameter sets and the mass sets of the GPU tests as value lists: every row of both tables, bit for bit
    rows = env_params_sets.set_rows(lib, vcfg)
    base = env_params.config_row(lib, vcfg)
    for g in range(env_params_sets.NUM_SETS):
        cfg_g = env_inertia_sets.set_cfg(env_params_sets.set_cfg(vcfg, g), g)
        spec = {"DAMPING": {"values": [float(rows[k, abi.VP_DAMPING]) for k in range(9)]}, "ACTION_DELAY": [0, g],
                "FPAM_K": [0.8, 1.0 + 0.02 * g], "CART_MASS": [0.3, 0.4 + 0.05 * g], "LINK_MASS": {"values": [0.9, 1.0, 1.1 + 0.01 * g]}}
        p, i = env_params.build_columns(spec, cfg_g, np.arange(70), 0, lib=lib)
        assert np.array_equal(bits(p), bits(env_params.build_table(spec, cfg_g, 42, 70, 0, lib=lib))), g
        assert np.array_equal(bits(i), bits(env_params.build_inertia_table(spec, cfg_g, 42, 70, 0, lib=lib))), g
    assert base.shape == (abi.VP_COUNT,)


def test_a_shard_equals_its_slice_and_every_column_passes_the_checks(lib, vcfg):
    k_all = (np.arange(2000) * 7) % 5
    p_all, i_all = env_params.build_columns(FULL, vcfg, np.arange(2000), k_all, lib=lib)
    p, i = env_params.build_columns(FULL, vcfg, np.arange(1000, 1070), k_all[1000:1070], lib=lib)
    assert np.array_equal(bits(p), bits(p_all[:, 1000:1070])) and np.array_equal(bits(i), bits(i_all[:, 1000:1070]))
    env_params.check_table(lib, vcfg, p_all)
    env_params.check_inertia_table(lib, vcfg, i_all)
    # episodes differ from one another, a number stays a number, a list's later episodes draw from the list
    p1, _ = env_params.build_columns(FULL, vcfg, np.arange(2000), 1, lib=lib)
    p2, _ = env_params.build_columns(FULL, vcfg, np.arange(2000), 2, lib=lib)
    assert np.mean(p1[abi.VP_DAMPING] != p2[abi.VP_DAMPING]) > 0.99
    assert (p1[abi.VP_RAIL_P_GAIN] == np.float32(9.0)).all() and (p2[abi.VP_RAIL_P_GAIN] == np.float32(9.0)).all()
    assert set(p1[abi.VP_SMOOTHING_ALPHA_DEFLATE].tolist()) == {np.float32(0.6), np.float32(0.75), np.float32(0.9)}
    p0, _ = env_params.build_columns(FULL, vcfg, np.arange(2000), 0, lib=lib)
    assert np.array_equal(p0[abi.VP_SMOOTHING_ALPHA_DEFLATE, :6], np.float32([0.6, 0.75, 0.9, 0.6, 0.75, 0.9]))       # the radix at 0
    assert not np.array_equal(p1[abi.VP_SMOOTHING_ALPHA_DEFLATE, :300], p0[abi.VP_SMOOTHING_ALPHA_DEFLATE, :300])     # not later


def test_integer_delay_ranges_hit_both_ends(lib, vcfg):
    for lo, hi in ((0, 8), (2, 3), (5, 5)):
        p, _ = env_params.build_columns({"ACTION_DELAY": [lo, hi]}, vcfg, np.repeat(np.arange(256), 4), np.tile(np.arange(1, 5), 256), lib=lib)
        d = p[abi.VP_ACTION_DELAY]
        assert d.min() == lo and d.max() == hi and np.array_equal(d, np.floor(d))


SEEDS, NAMES = (0, 42, 12345), ("DAMPING", "ACTION_DELAY", "FPAM_K", "LINK_MASS")


def test_statistics_of_the_per_episode_hash():
    """4096 envs x 16 episodes = 65536 draws per (seed, name).  Bounds: 5 sigma on the mean and on the correlations, the 0.999
    quantile of chi^2(8) on the nine delay values.  The reference formula was measured below 2 sigma and 15.3 on all of them:
    these bounds catch a broken mix, not bad luck."""
    g, k = np.meshgrid(np.arange(4096), np.arange(16), indexing="ij")
    n = g.size
    us = {}
    for seed in SEEDS:
        for name in NAMES:
            u = env_params.uniform01_episode(seed, name, g.ravel(), k.ravel()).reshape(g.shape)
            us[seed, name] = u
            assert u.min() >= 0.0 and u.max() < 1.0
            mean_err = abs(u.mean() - 0.5)
            print("seed %d %s: |mean - 0.5| = %.2e (bound %.2e)" % (seed, name, mean_err, 5 / np.sqrt(12 * n)))
            assert mean_err <= 5 / np.sqrt(12 * n)
            for what, a, b in (("consecutive episodes", u[:, :-1], u[:, 1:]), ("neighbouring envs", u[:-1], u[1:])):
                r = np.corrcoef(a.ravel(), b.ravel())[0, 1]
                print("  %s: r = %+.2e (bound %.2e)" % (what, r, 5 / np.sqrt(a.size)))
                assert abs(r) <= 5 / np.sqrt(a.size), (seed, name, what)
            counts = np.bincount(np.minimum(np.floor(u.ravel() * 9.0), 8).astype(np.int64), minlength=9)
            chi2 = float(((counts - n / 9.0) ** 2 / (n / 9.0)).sum())
            print("  chi^2(8) of the nine delay values: %.1f (bound 26.1)" % chi2)
            assert chi2 <= 26.1, (seed, name)
        for a, b in zip(NAMES[:-1], NAMES[1:]):                   # across names
            r = np.corrcoef(us[seed, a].ravel(), us[seed, b].ravel())[0, 1]
            assert abs(r) <= 5 / np.sqrt(n), (seed, a, b)


# ------------------------------------------------------------------------------------------------ the episode-log join
def test_ordinals_forwards_and_backwards_on_a_hand_made_log():
    """Three envs.  Env 0 finished episodes at steps 3, 9, 14; env 1 at 5 and 11 and was then reset from OUTSIDE (no row, no
    new episode: its counter stays 2); env 2 at 2, 4, 6, 8, 10.  Forward and backward counts agree on the whole log; with the
    ring having dropped the four oldest rows, counting backwards from the counters still names each survivor's episode, and
    counting forwards from zero does not."""
    env = np.array([2, 0, 2, 1, 2, 2, 0, 2, 1, 0])
    end = np.array([2, 3, 4, 5, 6, 8, 9, 10, 11, 14])
    counters = np.array([3, 2, 5])
    back = episodes.episode_ordinals(env, end, counters)
    forward = np.zeros(len(env), dtype=np.int64)
    seen = {}
    for j in np.argsort(end, kind="stable"):
        forward[j] = seen.get(env[j], 0)
        seen[env[j]] = forward[j] + 1
    assert np.array_equal(back, forward) and back.tolist() == [0, 0, 1, 0, 2, 3, 1, 4, 1, 2]
    shuffled = np.random.default_rng(0).permutation(len(env))     # the ring's order within a harvest means nothing
    assert np.array_equal(episodes.episode_ordinals(env[shuffled], end[shuffled], counters), back[shuffled])
    kept = np.arange(4, len(env))                                 # the ring dropped the four oldest rows
    assert episodes.episode_ordinals(env[kept], end[kept], counters).tolist() == back[kept].tolist() == [2, 3, 1, 4, 1, 2]
    forward_kept, seen = np.zeros(len(kept), dtype=np.int64), {}
    for j, r in enumerate(kept):
        forward_kept[j] = seen.get(env[r], 0)
        seen[env[r]] = forward_kept[j] + 1
    assert not np.array_equal(forward_kept, back[kept])
    assert episodes.episode_ordinals([], [], counters).shape == (0,)


def test_rows_gain_the_plant_of_their_episode_and_the_file_rebuilds_it(lib, vcfg, tmp_path):
    spec = {"DAMPING": [0.01, 0.05], "ACTION_DELAY": {"values": [0, 2]}, "LINK_MASS": [0.8, 1.3], "RAIL_P_GAIN": 9.0}
    rows = episodes.concat_rows([])
    R = 40
    rng = np.random.default_rng(1)
    rows = {name: (rng.integers(0, 7, R) if name in episodes.INT_COLUMNS else rng.uniform(size=R).astype(np.float32))
            for name in episodes.COLUMNS}
    rows["reached_ever"] = (rng.uniform(size=R) < 0.5).astype(np.float32)
    rows["episode"] = rng.integers(0, 4, R)
    offset = 1000
    p, i = env_params.build_columns(spec, vcfg, rows["env"] + offset, rows["episode"], lib=lib)
    out = episodes.with_episode_params(rows, p, abi.ENV_PARAM_ROW_NAMES, i)
    assert sorted(k for k in out if k.startswith("param_")) == ["param_ACTION_DELAY", "param_DAMPING", "param_LINK_MASS"]
    assert np.array_equal(out["param_DAMPING"], p[abi.VP_DAMPING]) and np.array_equal(out["param_LINK_MASS"], i[abi.VI_LINK_MASS0])
    values, rate, count = episodes.value_rate(out, "param_ACTION_DELAY")
    assert values.tolist() == [0.0, 2.0] and count.sum() == R
    path = str(tmp_path / "e.npz")
    episodes.save(path, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {"maxEpisodeLength": 12}, p[:, :7], abi.ENV_PARAM_ROW_NAMES, None, None,
                  redraw={"spec": spec, "seed": 42, "env_id_offset": offset, "base": env_params.config_row(lib, vcfg),
                          "inertia_base": env_params.inertia_config_row(lib, vcfg),
                          "geometry": (vcfg.link_length, vcfg.link_com, vcfg.gravity)})
    episode, columns = episodes.load_env_redraw(path)
    assert np.array_equal(episode, rows["episode"])
    p2, i2 = columns(episodes.load(path)[0]["env"], episode)
    assert np.array_equal(bits(p2), bits(p)) and np.array_equal(bits(i2), bits(i))
    plain = str(tmp_path / "plain.npz")
    episodes.save(plain, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {})
    assert episodes.load_env_redraw(plain) == (None, None)
