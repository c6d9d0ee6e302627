"""The device light record carries the two edges rectangleLight::sampleRay spans, B - A and D - A
(dt_scene_dev.h DLight::AB, AD; host_flatten.cpp), so that the light loop does not subtract them per lane, per
light, per step. They must be the f64 differences the kernel used to compute, bit for bit: every light of
final(240), and a rectangle light of a scaled, shifted synthetic scene, through dt_debug_light_edges (host
only, no device)."""
import ctypes

import numpy as np

import distraytracer_amd as dt
import scene_gen as sg


def _edges(built, g, n_lights):
    out = np.full((n_lights, 5, 3), np.nan)
    desc = built._ptr if isinstance(built, dt.BuiltScene) else ctypes.pointer(built)
    dt.check(dt.lib.dt_debug_light_edges(desc, ctypes.byref(g), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                         n_lights), "dt_debug_light_edges")
    return out


def _check(e, lights):
    for i in range(len(e)):
        for k, name in enumerate(("A", "B", "D")):
            assert np.array_equal(e[i, k], np.array(getattr(lights[i], name)[:])), (i, name)
    A, B, D, AB, AD = (e[:, k] for k in range(5))
    assert np.array_equal((B - A).view(np.uint64), AB.view(np.uint64))
    assert np.array_equal((D - A).view(np.uint64), AD.view(np.uint64))


def test_final_240_light_edges():
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    n = int(built.desc.n_lights)
    assert n > 0
    e = _edges(built, g, n)
    _check(e, built.desc.lights)
    rect = [i for i in range(n) if built.desc.lights[i].type == sg.RECT_LIGHT]
    assert rect and all(np.abs(e[i, 3:]).max() > 0 for i in rect)


def test_scaled_shifted_light_edges():
    desc, g, keep = sg.room(*sg.CASES["tiny-shifted"])
    e = _edges(desc, g, desc.n_lights)
    _check(e, desc.lights)
    assert np.abs(e[2, 3:]).max() > 0   # the rectangle light


def test_too_small_a_buffer_is_refused():
    desc, g, keep = sg.room()
    out = (ctypes.c_double * 15)()
    assert dt.lib.dt_debug_light_edges(ctypes.pointer(desc), ctypes.byref(g), out, 1) != 0
