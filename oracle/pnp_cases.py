"""The catalogue of track_motion inputs shared by tests/test_motion_reference_cpu.py (oracle vs
the longdouble reference, and the qualification that no decision hangs on rounding) and
tests/test_motion_edges_gpu.py (device vs oracle).  Test infrastructure.

Every case is rsvio.synthetic.motion_frame, then sliced, relabelled or moved:

  LM_CASES     every LM exit but one, rejected steps, step rotations past se3_plus_r's switch at
               |w| = 1/4, non-finite input, one to three features;
  POSE_CASES   the whole world moved by a rigid G, so that R_B_W of the last keyframe has a
               negative trace (quat_from_matrix's other branches on the host, pose_from7);
  COUNT_CASES  slices of one 2,140 + 2,140 feature frame at the join loop's stride edges
               (512 lanes x 2 per round), an empty camera on either side, the LDS cap of 4,096;
  JOIN_CASES   ids relabelled through an explicit old -> new mapping (geometry untouched) so that
               the hash table's probe runs, wrap-around, free-slot and exhausted misses, both key
               words and the id 2^64 - 1 decide lookups;
  remap_sequence()  four maps in a row for one handle.

LM_TRUST_REGION is NOT covered.  From lambda = 1e-4 the exit needs 15 rejected steps in a row
(lambda *= nu, nu doubling), and no input is known on which the oracle gets there with every
decision away from rounding: as lambda grows the step shrinks until its cost change is within the
cost tolerance, and that test comes first.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from . import pnp_reference as PR

TOP_ID = PR.TOP_ID


@dataclass
class PnpCase:
    name: str
    ids_l: np.ndarray
    uv_l: np.ndarray
    ids_r: np.ndarray
    uv_r: np.ndarray
    map_ids: np.ndarray
    map_pw: np.ndarray
    T_last: np.ndarray
    T_C_B2: np.ndarray
    cfg: dict = field(default_factory=dict)   # keyword arguments of lm_cfg / pnp_cfg
    expect: tuple | None = None               # (status, iterations) of the oracle, where the case fixes it
    n_obs: int | None = None                  # the observation count the case is built for
    nonfinite: bool = False                   # both costs non-finite, compare by isfinite
    same_as: str | None = None                # the case whose result this one must reproduce
    stats: dict | None = None                 # map_stats() the case is built for
    facts: dict = field(default_factory=dict)  # what else the builder promises (checked on the CPU)

    def args(self):
        """Positional arguments of oracle.track_motion / track_motion_ref up to the cfg."""
        return (self.ids_l, self.uv_l, self.ids_r, self.uv_r, self.map_ids, self.map_pw, self.T_last, self.T_C_B2)


def _S():
    from rsvio import synthetic
    return synthetic


def _case(name, m, **kw):
    return PnpCase(name, m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.map_ids, m.map_pw, m.T_W_B_last_kf, m.T_C_B2, **kw)


@functools.lru_cache(maxsize=None)
def _frame(**kw):
    return _S().motion_frame(**kw)


def _default():
    return _frame(seed=1)


# ---- LM branches --------------------------------------------------------------------------------

def _big_rot(seed, rot, max_it, expect):
    return lambda name: _case(name, _frame(seed=seed, n_map=400, n_feat=120, step=(0.3, rot)),
                              cfg=dict(max_iterations=max_it), expect=expect)


def _poisoned(value, matched):
    """One left feature's u replaced; `matched`: the feature has a map point."""
    def build(name):
        m = _default()
        hit = np.isin(m.ids_l, m.map_ids)
        j = np.nonzero(hit if matched else ~hit)[0][3]
        uv = m.uv_l.copy()
        uv[j, 0] = value
        m2 = dataclasses.replace(m, uv_l=uv)
        if matched:
            return _case(name, m2, expect=(-1, 1), nonfinite=True, n_obs=600)
        return _case(name, m2, expect=(1, 3), n_obs=600, same_as="clean")
    return build


def _tiny(n_feat, drop_right=False):
    def build(name):
        m = _frame(seed=1, n_map=50, n_feat=n_feat, unmapped=0)
        if drop_right:
            m = dataclasses.replace(m, ids_r=m.ids_r[:0], uv_r=m.uv_r[:0])
        expect = {(1, False): (1, 6), (2, False): (1, 6), (3, False): (1, 3), (1, True): (2, 3)}[(n_feat, drop_right)]
        return _case(name, m, expect=expect, n_obs=n_feat * (1 if drop_right else 2))
    return build


def _cfg_case(expect, **cfg):
    return lambda name: _case(name, _default(), cfg=cfg, expect=expect, n_obs=600)


LM_CASES = {
    "clean": _cfg_case((1, 3)),
    "big-rot-A": _big_rot(3, 0.4, 10, (3, 10)),
    "big-rot-A30": _big_rot(3, 0.4, 30, (1, 16)),
    "big-rot-B": _big_rot(3, 0.6, 10, (3, 10)),
    "big-rot-B30": _big_rot(3, 0.6, 30, (1, 21)),
    "big-rot-C": _big_rot(2, 0.9, 30, (1, 15)),
    "sincos-only": _big_rot(1, 0.3, 10, (1, 5)),
    "param-tol": _cfg_case((2, 2), cost_tolerance=0.0, parameter_tolerance=1e-2),
    "param-tol-0": _cfg_case((2, 1), lambda_init=1e30),
    "max-iter-1": _cfg_case((3, 1), max_iterations=1),
    "max-iter-0": _cfg_case((3, 0), max_iterations=0),
    "linsolve": _cfg_case((-3, 1), lambda_init=-1e9),
    "numfail-nan": _poisoned(np.nan, True),
    "numfail-inf": _poisoned(np.inf, True),
    "nan-unmatched": _poisoned(np.nan, False),
    "inf-unmatched": _poisoned(np.inf, False),
    "tiny-1": _tiny(1),
    "tiny-2": _tiny(2),
    "tiny-3": _tiny(3),
    "tiny-1-left-only": _tiny(1, drop_right=True),
}


# ---- poses --------------------------------------------------------------------------------------

def _moved(G):
    def build(name):
        m = _default()
        pw = (m.map_pw.astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
        m2 = dataclasses.replace(m, map_pw=pw, T_W_B_last_kf=G @ m.T_W_B_last_kf)
        R_BW = m2.T_W_B_last_kf[:3, :3].T
        return _case(name, m2, n_obs=600, facts=dict(trace=float(np.trace(R_BW))))
    return build


def _rot3(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    G = np.eye(4)
    G[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    return G


POSE_CASES = {
    "world-rot-3rad": _moved(_rot3(np.random.default_rng(21).normal(size=3), 3.0)),
    "world-rot-180x": _moved(np.diag([1.0, -1.0, -1.0, 1.0])),
}


# ---- feature counts -----------------------------------------------------------------------------

COUNTS = [(1, 0), (0, 1), (1, 1), (63, 1), (64, 64), (511, 0), (512, 0), (256, 257), (1023, 0), (512, 512),
          (513, 512), (2048, 2047), (2048, 2048), (2140, 1956), (0, 2140)]


def _count(n_l, n_r):
    def build(name):
        m = _frame(seed=5, n_map=2300, n_feat=2100)
        assert len(m.ids_l) == 2140 and len(m.ids_r) == 2140
        m2 = dataclasses.replace(m, ids_l=m.ids_l[:n_l], uv_l=m.uv_l[:n_l], ids_r=m.ids_r[:n_r], uv_r=m.uv_r[:n_r])
        n_obs = int(np.isin(m2.ids_l, m.map_ids).sum() + np.isin(m2.ids_r, m.map_ids).sum())
        return _case(name, m2, n_obs=n_obs)
    return build


def _duplicate(name):
    """A matched left feature listed twice (the same id, another observation): two factors."""
    m = _frame(seed=1, n_map=64, n_feat=30)
    j = np.nonzero(np.isin(m.ids_l, m.map_ids))[0][5]
    ids = np.insert(m.ids_l, j + 1, m.ids_l[j])
    uv = np.insert(m.uv_l, j + 1, m.uv_l[j] + np.float32(1e-3), axis=0)
    return _case(name, dataclasses.replace(m, ids_l=ids, uv_l=uv), n_obs=61)


COUNT_CASES = {f"n{a}+{b}": _count(a, b) for a, b in COUNTS}
COUNT_CASES["duplicate-id"] = _duplicate


# ---- the join -----------------------------------------------------------------------------------

def _small():
    """64 map points, all seen by both cameras, plus 40 features per camera without a map point."""
    m = _frame(seed=1, n_map=64, n_feat=64)
    assert len(m.ids_l) == 104 and len(m.ids_r) == 104
    return m


def _relabel(m, mapping, drop=()):
    """ids through old -> new (ids not in the mapping stay); `drop`: old map ids taken out of the
    map (their features stay, under their new ids).  Map and feature lists re-sorted by id."""
    f = np.vectorize(lambda i: mapping.get(int(i), int(i)), otypes=[np.uint64])
    keep = ~np.isin(m.map_ids, np.array(list(drop), np.uint64))
    mid = f(m.map_ids[keep])
    assert len(set(mid.tolist())) == len(mid)
    o = np.argsort(mid, kind="stable")
    out = dict(map_ids=mid[o], map_pw=m.map_pw[keep][o])
    for s in ("l", "r"):
        ids = f(getattr(m, "ids_" + s))
        o = np.argsort(ids, kind="stable")
        out["ids_" + s] = ids[o]
        out["uv_" + s] = getattr(m, "uv_" + s)[o]
    return dataclasses.replace(m, **out)


def ids_in_bucket(bucket, mask, count, start=1, exclude=()):
    """The first `count` integers >= start that hash to `bucket` (brute force)."""
    out, i, exclude = [], start, set(int(e) for e in exclude)
    while len(out) < count:
        block = np.arange(i, i + 4096, dtype=np.uint64)
        for v in block[PR.map_bucket_array(block, mask) == bucket].tolist():
            if v not in exclude and len(out) < count:
                out.append(v)
        i += 4096
    return out


def _collide(n_in_map):
    """n_in_map map ids that all hash to bucket 63 of 64: the run wraps 63 -> 0 -> ... ; the other
    24 + map points leave the map, half of their features relabelled to further ids of bucket 63
    (misses that walk the run), half to ids of bucket 32 (empty: a miss at depth 0)."""
    def build(name):
        m = _small()
        old = m.map_ids.tolist()
        inmap, out = old[:n_in_map], old[n_in_map:]
        c63 = ids_in_bucket(63, 63, n_in_map + len(out) // 2, start=100000)
        c32 = ids_in_bucket(32, 63, len(out) - len(out) // 2, start=100000)
        mapping = dict(zip(inmap, c63[:n_in_map]))
        mapping.update(zip(out[:len(out) // 2], c63[n_in_map:]))
        mapping.update(zip(out[len(out) // 2:], c32))
        m2 = _relabel(m, mapping, drop=out)
        full = n_in_map % PR.BUCKET == 0
        return _case(name, m2, n_obs=2 * n_in_map,
                     stats=dict(buckets=64, max_probe=(n_in_map - 1) // PR.BUCKET, has_top=0, n_map=n_in_map),
                     facts=dict(miss_run=c63[n_in_map:], miss_empty=c32, miss_run_end="exhausted" if full else "free"))
    return build


def _word_halves(name):
    m = _small()
    old = m.map_ids.tolist()
    up = 5 << 32                                       # every id gets a high word
    mapping = {i: i + up for i in old}
    mapping.update({int(i): int(i) + up for i in np.concatenate([m.ids_l, m.ids_r]).tolist()})
    mask = 63                                          # 62 map ids -> 64 buckets
    # two ids with the same low word in one bucket, two with the same high word in one bucket
    lo = 0x1234ABCD
    by_bucket = {}
    a = None
    for h in range(6, 4096):
        v = (h << 32) | lo
        b = PR.map_bucket(v, mask)
        if b in by_bucket:
            a = (by_bucket[b], v)
            break
        by_bucket[b] = v
    hi = 0x77 << 32
    by_bucket = {}
    bpair = None
    for l in range(1, 4096):
        v = hi | l
        b = PR.map_bucket(v, mask)
        if b in by_bucket:
            bpair = (by_bucket[b], v)
            break
        by_bucket[b] = v
    # map points 10, 11 -> a[0], bpair[0]; map points 12, 13 leave the map, their features
    # become a[1], bpair[1]
    mapping[old[10]], mapping[old[11]] = a[0], bpair[0]
    mapping[old[12]], mapping[old[13]] = a[1], bpair[1]
    m2 = _relabel(m, mapping, drop=(old[12], old[13]))
    return _case(name, m2, n_obs=2 * 62, stats=dict(buckets=64, has_top=0, n_map=62),
                 facts=dict(same_low=a, same_high=bpair))


def _top_in_map(name):
    m = _small()
    m2 = _relabel(m, {int(m.map_ids[-1]): TOP_ID})
    return _case(name, m2, n_obs=128, same_as="small", stats=dict(buckets=64, has_top=1, n_map=64))


def _top_in_features(name):
    m = _small()
    stray = int(m.ids_l[~np.isin(m.ids_l, m.map_ids)][0])
    m2 = _relabel(m, {stray: TOP_ID})
    return _case(name, m2, n_obs=128, same_as="small", stats=dict(buckets=64, has_top=0, n_map=64))


JOIN_CASES = {
    "small": lambda name: _case(name, _small(), n_obs=128, stats=dict(buckets=64, has_top=0, n_map=64)),
    "collide-full": _collide(40),
    "collide-partial": _collide(38),
    "word-halves": _word_halves,
    "top-id": _top_in_map,
    "top-id-features-only": _top_in_features,
}


def remap_sequence():
    """[(label, map_ids, map_pw)] to set on ONE handle in this order, and the frame to run after
    each: its features include ids that are in the 9,000-id map only."""
    m = _frame(seed=11, n_map=9000, n_feat=800)
    seen = np.nonzero(np.isin(m.map_ids, m.ids_l))[0]
    few = seen[::len(seen) // 40][:40]
    e = (m.map_ids[:0], m.map_pw[:0])
    return m, [("9000", m.map_ids, m.map_pw), ("40", m.map_ids[few], m.map_pw[few]), ("0",) + e,
               ("9000-again", m.map_ids, m.map_pw)]


GROUPS = {"lm": LM_CASES, "pose": POSE_CASES, "count": COUNT_CASES, "join": JOIN_CASES}


@functools.lru_cache(maxsize=None)
def get(group, name) -> PnpCase:
    return GROUPS[group][name](name)
