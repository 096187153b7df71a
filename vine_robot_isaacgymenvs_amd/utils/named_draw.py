"""Named draws: a small set of named values per env or plant, each written in a config as

  a number               everybody gets it;
  ``[lo, hi]``           uniform (for an INTEGER name: over the integers lo..hi, both ends included);
  ``{values: [v0, ..]}`` a value list: in episode 0 the lists of one spec together count the global id in a mixed radix, the
                         first list being the fastest digit; from episode 1 on each list draws its own index.

What id ``g`` gets in episode ``k`` is a pure function of ``(seed, name, g, k)``: ``redraw_value`` of csrc/vine_named_draw.h
on the device, ``draw`` here, bit for bit.  ENV_PARAMS (per episode and under ADR), ENV_SENSOR, ENV_PUSH, ENV_TARGET and the
planner's ``observe=`` / ``filter=`` all state their draw as a list of ``(draw name, form)`` and call this module: the parser
(``form``), what a form can give (``candidates``, ``varying``), the draw, its packing into ``abi.VineEnvRedrawName`` slots
(``pack``) and the episode log's ``param_*`` columns (``episode_params``).  ``philox4x32_10`` is here because the launches
that ride on these draws (sensor, push, planner) restate their per-step streams with it."""
import hashlib

import numpy as np

from .. import abi
from .config import ConfigError


# ---- the hash
def mix(x):
    """splitmix64's finaliser on uint64 arrays."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def name_key(name):
    """The 64-bit key of a name: the first 8 bytes of its SHA-256, little endian."""
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little")


def uniform01_episode(seed, name, gids, episodes):
    """One float64 in [0, 1) per (global id, episode) pair, a pure function of ``(seed, name, id, episode)``; episode 0 mixes
    nothing in, because ``mix(0) == 0``."""
    g = np.asarray(gids, dtype=np.uint64)
    k = np.asarray(episodes, dtype=np.uint64)
    with np.errstate(over="ignore"):
        pre = mix(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(name_key(name))) + g * np.uint64(0x9E3779B97F4A7C15)
        h = mix(pre ^ mix(k))
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint32 arrays (broadcast against each other): the four output words."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & m32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return [x.astype(np.uint32) for x in c]


# ---- a config entry as a form
def number(where, v, finite=True):
    """``v`` as a float; ``finite``: also refuse NaN and the infinities."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or (finite and not np.isfinite(v)):
        raise ConfigError("%s: %r is not a %snumber" % (where, v, "finite " if finite else ""))
    return float(v)


def form(where, entry, finite=True):
    """A config entry as a plain number, ``[lo, hi]`` or ``{"values": [..]}`` of floats: what the episode files store as
    JSON.  ``where`` names the key in a ``ConfigError``; ``finite`` as for ``number``."""
    if hasattr(entry, "keys"):
        if list(entry.keys()) != ["values"]:
            raise ConfigError("%s: a mapping must hold the one key 'values', not %s" % (where, sorted(entry.keys())))
        vals = entry["values"]
        if not isinstance(vals, (list, tuple)) or len(vals) == 0:
            raise ConfigError("%s: 'values' must be a non-empty list" % where)
        return {"values": [number(where, v, finite) for v in vals]}
    if isinstance(entry, (list, tuple)):
        if len(entry) != 2:
            raise ConfigError("%s: a range is [lo, hi], not %r" % (where, list(entry)))
        lo, hi = number(where, entry[0], finite), number(where, entry[1], finite)
        if lo > hi:
            raise ConfigError("%s: lo > hi in [%g, %g]" % (where, lo, hi))
        return [lo, hi]
    return number(where, entry, finite)


def flag(where, v):
    """A config bool (``PER_EPISODE``, ``COMPENSATE``) as a ``bool``."""
    if not isinstance(v, (bool, np.bool_)):
        raise ConfigError("%s must be a bool, not %r" % (where, v))
    return bool(v)


def candidates(form):
    """What a form CAN give: both ends of a range, every listed value, the number."""
    return list(form["values"]) if isinstance(form, dict) else list(form) if isinstance(form, (list, tuple)) else [form]


def varying(names, spec):
    """The names of ``names`` whose value in ``spec`` can differ between ids or episodes."""
    return [n for n in names if len(set(candidates(spec[n]))) > 1]


# ---- the draw
def draw(named_forms, seed, gids, episodes, integer=(), who="draw"):
    """float64 [S, M]: the values of the S ``(draw name, form)`` pairs of ``named_forms``, in their order (the order of the
    mixed radix), for M ``(global id, episode)`` pairs; ``integer``: the draw names whose range is over the integers.
    ``ValueError``, in the name of ``who``, for a negative id or episode."""
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    k = np.broadcast_to(np.asarray(episodes, dtype=np.int64), gids.shape)
    if np.any(gids < 0) or np.any(k < 0):
        raise ValueError("%s: env ids and episodes are non-negative" % who)
    out, radix = np.zeros((len(named_forms), len(gids)), dtype=np.float64), 1
    for s, (name, f) in enumerate(named_forms):
        if isinstance(f, dict):
            vals = np.asarray(f["values"], dtype=np.float64)
            u = uniform01_episode(seed, name, gids, k)
            later = np.minimum(np.floor(u * float(len(vals))).astype(np.int64), len(vals) - 1)
            out[s] = vals[np.where(k == 0, (gids // radix) % len(vals), later)]
            radix *= len(vals)
        elif isinstance(f, (list, tuple)):
            lo, hi = np.float64(f[0]), np.float64(f[1])
            u = uniform01_episode(seed, name, gids, k)
            out[s] = np.minimum(lo + np.floor(u * (hi - lo + 1.0)), hi) if name in integer else lo + (hi - lo) * u
        else:
            out[s] = np.float64(f)
    return out


def pack(named_forms, count=None, slot=None):
    """``(abi.VineEnvRedrawName * count, values float64 [V])`` of ``(draw name, form)`` pairs: per name its form, ends, key, the
    extent of its list in ``values`` and its place in the mixed radix.  ``slot(name)``: where a name goes (default: in order,
    ``count`` = their number); a slot nobody fills stays ABSENT."""
    names = (abi.VineEnvRedrawName * (len(named_forms) if count is None else count))()
    values, radix = [], 1
    for s, (name, f) in enumerate(named_forms):
        nm = names[s if slot is None else slot(name)]
        nm.key, nm.radix = name_key(name), 1
        if isinstance(f, dict):
            nm.form, nm.values_first, nm.values_count, nm.radix = abi.REDRAW_VALUES, len(values), len(f["values"]), radix
            values += list(f["values"])
            radix *= len(f["values"])
        elif isinstance(f, (list, tuple)):
            nm.form, nm.lo, nm.hi = abi.REDRAW_RANGE, f[0], f[1]
        else:
            nm.form, nm.lo, nm.hi = abi.REDRAW_NUMBER, f, f
    return names, np.asarray(values, dtype=np.float64)


def named(names, draw_names, spec):
    """The ``(draw name, form)`` pairs of a checked spec whose keys are ``names``."""
    return [(d, spec[n]) for n, d in zip(names, draw_names)]


def episode_params(names, draw_names, spec, seed, gids, episodes, integer=()):
    """``{draw name: float32 [M]}`` of the names that vary: what the ``param_<draw name>`` columns of the episode log hold for
    rows of global envs ``gids`` in ``episodes`` (episode 0's draw where the values are held: no ``PER_EPISODE``)."""
    drawn = draw(named(names, draw_names, spec), seed, gids, episodes if spec["PER_EPISODE"] else 0, integer).astype(np.float32)
    return {draw_names[names.index(n)]: drawn[names.index(n)] for n in varying(names, spec)}
