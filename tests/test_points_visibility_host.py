"""Mutual visibility of two point sets (include/dt.h dt_points_visibility), what needs no GPU: the exports and
constants, every argument check that comes before the scene is looked at (shown as tests/test_aux_args_host.py shows
it: a stand-in scene that is never dereferenced, and the caller's stats left alone), visibility_matrix against the
packing rule, and what the point sets of tests/points_visibility_ref.py exercise, by the restatement alone."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd._lib import DT_PVIS_TILE, EXPORTS, Visibility, VisibilityParams
from points_visibility_ref import N_A, N_B, TILE, case, classes, pack, reference

INVALID = -1
N = 5
STAND_IN = ctypes.c_void_p(0x1000)   # a scene that is never dereferenced


def test_exports_and_constants():
    for name in ("dt_points_visibility", "dt_visibility_params_default"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    assert DT_PVIS_TILE == TILE == 256 and DT_PVIS_TILE % 32 == 0
    # dt_visibility_params: three pointers and falloff (padded); dt_visibility: four pointers
    assert ctypes.sizeof(VisibilityParams) == 32 and VisibilityParams.falloff.offset == 24
    assert [f for f, _ in Visibility._fields_] == list(dt.VISIBILITY_PLANES) == ["bits", "count_a", "count_b", "weight_a"]
    p = VisibilityParams()
    ctypes.memset(ctypes.byref(p), 0x5A, ctypes.sizeof(p))
    dt.lib.dt_visibility_params_default(ctypes.byref(p))
    assert (p.skip_b, p.normal_a, p.normal_b, p.falloff) == (None, None, None, 0)
    dt.lib.dt_visibility_params_default(None)   # tolerated, as the other defaults


# ---- the argument checks, before any device work --------------------------------------------------------------

_KEEP = []


def _arr(n, dtype=np.float64):
    a = np.zeros(n, dtype)
    _KEEP.append(a)
    return a


def _planes(*wanted):
    return Visibility(*[_arr(8 * N).ctypes.data if w else None for w in wanted])


def _params(normal_a=True, normal_b=True, falloff=0):
    p = VisibilityParams()
    p.skip_b = _arr(N, np.int32).ctypes.data
    p.normal_a = _arr(3 * N).ctypes.data if normal_a else None
    p.normal_b = _arr(3 * N).ctypes.data if normal_b else None
    p.falloff = falloff
    return p


OKAY = dict(scene=STAND_IN, g=dt.globals_default(), n_a=N, a=_arr(3 * N), n_b=N, b=_arr(3 * N), p=_params(),
            out=_planes(1, 1, 1, 1))
W = "dt_points_visibility: "
ROWS = [
    (dict(scene=None), W + "null scene"),
    (dict(g=None), W + "null globals"),
    (dict(a=None), W + "null a"),
    (dict(b=None), W + "null b"),
    (dict(p=None), W + "null params"),
    (dict(out=None), W + "null out"),
    (dict(out=Visibility()), W + "out wants no plane (every pointer is null)"),
    (dict(n_a=-1), W + "n_a < 0"),
    (dict(n_b=-1), W + "n_b < 0"),
    (dict(n_a=2 ** 31), W + "n_a >= 2^31"),
    (dict(n_b=2 ** 31), W + "n_b >= 2^31"),
    (dict(n_a=2 ** 40), W + "n_a >= 2^31"),
    (dict(p=_params(normal_a=False)), W + "out->weight_a given without params->normal_a"),
    (dict(p=_params(normal_b=False)), W + "out->weight_a given without params->normal_b"),
    (dict(p=_params(normal_a=False, normal_b=False)), W + "out->weight_a given without params->normal_a"),
    (dict(p=_params(falloff=-1)), W + "falloff -1 outside 0..1"),
    (dict(p=_params(falloff=2)), W + "falloff 2 outside 0..1"),
    # two faults: the order of the checks
    (dict(scene=None, out=None), W + "null scene"),
    (dict(b=None, n_a=-1), W + "null b"),
    (dict(out=Visibility(), n_b=-1), W + "out wants no plane (every pointer is null)"),
    (dict(n_a=-1, n_b=2 ** 31), W + "n_a < 0"),
    (dict(n_b=2 ** 31, p=_params(falloff=2)), W + "n_b >= 2^31"),
    (dict(p=_params(normal_b=False, falloff=2)), W + "out->weight_a given without params->normal_b"),
    # ... and the errors come before the "no pairs" shortcut
    (dict(n_a=0, p=_params(falloff=2)), W + "falloff 2 outside 0..1"),
    (dict(n_b=0, out=Visibility()), W + "out wants no plane (every pointer is null)"),
    (dict(n_a=0, n_b=0, p=_params(normal_a=False)), W + "out->weight_a given without params->normal_a"),
]


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_rejected_before_any_device_work(i):
    change, text = ROWS[i]
    kw = dict(OKAY, **change)
    st = dt.Stats()
    ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
    ref = lambda x: None if x is None else ctypes.byref(x)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rc = dt.lib.dt_points_visibility(kw["scene"], ref(kw["g"]), kw["n_a"], ptr(kw["a"]), kw["n_b"], ptr(kw["b"]),
                                     ref(kw["p"]), ref(kw["out"]), 0, None, ctypes.byref(st))
    assert rc == INVALID, (change, dt.lib.dt_last_error())
    assert dt.lib.dt_last_error() == text.encode(), change
    assert bytes(st) == b"\x5a" * ctypes.sizeof(st), change   # a rejected call leaves the caller's stats alone


def test_normals_are_needed_for_the_weight_alone():
    """without weight_a the call passes every argument check with no normals: it gets as far as the scene, which a
    null scene shows without touching a device"""
    st = dt.Stats()
    p = _params(normal_a=False, normal_b=False)
    out = _planes(1, 1, 1, 0)
    a, b = _arr(3 * N), _arr(3 * N)
    rc = dt.lib.dt_points_visibility(None, ctypes.byref(dt.globals_default()), N, a.ctypes.data, N, b.ctypes.data,
                                     ctypes.byref(p), ctypes.byref(out), 0, None, ctypes.byref(st))
    assert rc == INVALID and dt.lib.dt_last_error() == (W + "null scene").encode()


def test_the_wrapper_rejects_what_it_can_see():
    pts = np.zeros((2, 3))
    g = dt.globals_default()
    with pytest.raises(dt.DTError, match="unknown plane 'light'"):
        dt.points_visibility(None, g, pts, pts, planes=("light",))
    with pytest.raises(dt.DTError, match="weight_a needs normals_a and normals_b"):
        dt.points_visibility(None, g, pts, pts, normals_a=pts, planes=("weight_a",))
    with pytest.raises(dt.DTError, match="3 doubles per point"):
        dt.points_visibility(None, g, np.zeros(4), pts)
    with pytest.raises(dt.DTError, match="skip_b holds 3 elements, 2 rays need 2"):
        dt.points_visibility(None, g, pts, pts, skip_b=np.zeros(3, np.int32))
    with pytest.raises(dt.DTError, match=r"dt_points_visibility failed \(-1\): dt_points_visibility: null scene"):
        dt.points_visibility(None, g, pts, pts)


# ---- the bit matrix -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_a,n_b", [(1, 1), (3, 31), (2, 32), (5, 33), (4, 64), (7, 293)])
def test_visibility_matrix_round_trips(n_a, n_b):
    rng = np.random.default_rng(1000 * n_a + n_b)
    vis = rng.random((n_a, n_b)) < 0.5
    vis[0, n_b - 1] = True
    bits = pack(vis)
    words = (n_b + 31) // 32
    assert bits.shape == (n_a, words) and bits.dtype == np.uint32
    # the rule of include/dt.h, entry by entry
    for i in range(n_a):
        for j in range(n_b):
            assert bool((int(bits[i, j >> 5]) >> (j & 31)) & 1) == bool(vis[i, j])
    if n_b % 32:   # the unused high bits of a row's last word are 0
        assert (bits[:, -1] >> np.uint32(n_b % 32) == 0).all()
    got = dt.visibility_matrix(bits, n_b)
    assert got.dtype == bool and got.shape == (n_a, n_b) and np.array_equal(got, vis)
    # the same bits as int32 (what torch holds) and flat
    assert np.array_equal(dt.visibility_matrix(bits.view(np.int32), n_b), vis)
    assert np.array_equal(dt.visibility_matrix(bits.reshape(-1), n_b), vis)
    assert np.array_equal(pack(got), bits)


def test_visibility_matrix_of_nothing():
    assert dt.visibility_matrix(np.zeros((3, 0), np.uint32), 0).shape == (3, 0)
    assert dt.visibility_matrix(np.zeros((0, 2), np.uint32), 40).shape == (0, 40)


# ---- what the point sets exercise, by the restatement alone ---------------------------------------------------

def test_the_point_sets_exercise_every_class():
    c = classes()
    print(c)
    a, na, b, nb, skip, desc, g, keep, panel = case()
    assert (len(a), len(b)) == (N_A, N_B) == (64 * 2 + 7, 256 + 37)
    assert c["live_pairs"] == (N_A - 1) * (N_B - 1)
    assert c["visible"] + c["hidden"] == c["live_pairs"]
    assert 10 * c["visible"] >= c["live_pairs"] and 10 * c["hidden"] >= c["live_pairs"]
    assert c["hidden_only_without_skip"] >= 1      # hidden by the panel, and only because skip_b is -1
    assert c["visible_only_with_skip"] >= 1        # the panel would hide its own texel
    assert c["mixed_words"] >= 1                   # 0s and 1s inside one full word
    assert c["void_sources"] == 1 and c["void_targets"] == 1
    assert c["void_ray_pairs"] == 1 and c["void_ray_pair_visible"]
    assert c["weight_in_both_tiles"] >= 1
    assert c["falloff_changes_weight"] >= 1
    assert (skip[:280] == panel).all() and (skip[280:] == -1).all()


def test_the_prediction_is_consistent_with_itself():
    """rows, columns and the split of the targets, on the restatement: what the GPU tests then ask of the device"""
    ref, none, allp = reference()
    full, traced = ref.planes(1)
    vis = dt.visibility_matrix(full["bits"], N_B)
    assert np.array_equal(full["count_a"], vis.sum(axis=1)) and np.array_equal(full["count_b"], vis.sum(axis=0))
    assert traced == (N_A - 1) * (N_B - 1) - 1
    assert not vis[96].any() and not vis[:, 100].any() and full["weight_a"][96] == 0
    left, tl = ref.planes(1, cols=slice(0, TILE))
    right, tr = ref.planes(1, cols=slice(TILE, N_B))
    assert tl + tr == traced
    assert np.array_equal(np.hstack([dt.visibility_matrix(left["bits"], TILE), dt.visibility_matrix(right["bits"], N_B - TILE)]), vis)
    assert np.array_equal(left["count_a"] + right["count_a"], full["count_a"])
    # the fixed order: (0.0 + tile 0) + tile 1, bit for bit
    assert (left["weight_a"] + right["weight_a"]).tobytes() == full["weight_a"].tobytes()
    assert (full["weight_a"] > 0).any()
