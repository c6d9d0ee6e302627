// dt_device.h — the kernels' device library for the auxiliary units: build knobs, math and sky, RNG,
// shape tests, tree and list walks, shading (Entry, Counters, Ctx, run_pass), pixel and camera, DLaunch. For now the
// library is the part of dt_kernels.hip above its own kernels, taken in as it stands there, in its order (the order
// is part of the code generation); the units name only this header, so the library can move into headers of its
// own without touching them.
#pragma once
#define DT_LIBRARY_ONLY 1
#include "dt_kernels.hip"
