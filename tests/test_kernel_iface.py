"""The host/kernel boundary is declared once (distraytracer_amd/csrc/dt_kernel_iface.h): every kernel unit
(dt_kernels.hip and one .hip per auxiliary kernel family, the Makefile's SRC_* list) includes the header, so a
definition that disagrees with its declaration does not compile; the two host units declare none of its symbols
themselves; and every such extern "C" function a kernel unit defines is in the header.
Plain regular expressions over the sources. No GPU."""
import os
import re
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distraytracer_amd", "csrc")
# the names of the boundary: launch wrappers, kernel pointers, the trace builds' trios, the record's layout
IFACE = re.compile(r"^(dt_launch_\w+|\w+_kernel_ptr|dt_trace_kernel\w*|dt_launch_size|\w+_struct_(offset|size))$")
# an extern "C" function: a declaration or a definition, up to its parameter list
EXTERN_C = re.compile(r'extern\s+"C"\s+(?!__global__)[\w\s\*]*?\b(\w+)\s*\(')


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def extern_c_names(text):
    return {m.group(1) for m in EXTERN_C.finditer(text)}


def test_the_pattern_finds_declarations():
    text = 'extern "C" hipError_t dt_launch_x(const void* a,\n int b);\nextern "C" const void* dt_y_kernel_ptr(int k)\n{'
    assert extern_c_names(text) == {"dt_launch_x", "dt_y_kernel_ptr"}
    assert all(IFACE.match(n) for n in ("dt_launch_x", "dt_y_kernel_ptr", "dt_trace_kernel_w5_launch", "dt_launch_size",
                                        "dt_scene_struct_offset", "dt_scene_struct_size"))
    assert not IFACE.match("dt_render") and not IFACE.match("dt_repro_launch")


def test_the_host_units_declare_no_interface_symbol():
    for name in ("dt_api.cpp", "dt_api_aux.cpp"):
        text = read(name)
        assert '#include "dt_api_internal.h"' in text, name
        own = sorted(n for n in extern_c_names(text) if IFACE.match(n))
        assert own == [], (name, own)
        # ... nor through a macro over the list of trace builds, as dt_api.cpp once did
        assert not re.search(r'extern\s+"C"[^\n;]*##', text), name
    assert '#include "dt_kernel_iface.h"' in read("dt_api_internal.h")


def kernel_units():
    """dt_kernels.hip and the unit of every auxiliary build (Makefile AUX_BUILDS, SRC_<build>)."""
    def var(name):
        return subprocess.check_output(["make", "-s", "-C", CSRC, "var-" + name], text=True).split()
    aux = var("AUX_BUILDS")
    assert len(aux) == 14
    units = []
    for b in aux:
        src = var("SRC_" + b)
        assert len(src) == 1 and src[0].endswith(".hip"), b
        units.append(src[0])
    assert len(set(units)) == 13, "one unit per family, dt_points_occl.hip built twice"
    return ["dt_kernels.hip"] + sorted(set(units))


def test_every_interface_function_the_kernels_define_is_declared_in_the_header():
    header = read("dt_kernel_iface.h")
    declared = extern_c_names(header)
    defined = set()
    for unit in kernel_units():
        text = read(unit)
        assert re.search(r'^#include "dt_kernel_iface.h"$', text, re.M), unit
        assert not re.search(r"^#if", text[:text.index('#include "dt_kernel_iface.h"')], re.M), (unit, "included in every build")
        own = {n for n in extern_c_names(text) if IFACE.match(n)}
        assert own, unit
        assert not (own & defined), (unit, sorted(own & defined))
        defined |= own
    assert len(defined) >= 30
    assert sorted(defined - declared) == []
    hip = read("dt_kernels.hip")
    # the trace builds' trio is defined through DT_CAT(DT_TRACE_KERNEL, _launch | _ptr | _traits), DT_TRACE_KERNEL
    # being the build's kernel name (the Makefile's -DDT_KNAME, DT_WINDOW's _win / _awin): the header declares the
    # trio for every name of its list in all three modes
    for sfx in ("_launch", "_ptr", "_traits"):
        assert re.search(r'extern "C" [\w\s\*]*DT_CAT\(DT_TRACE_KERNEL, %s\)' % sfx, hip), sfx
        assert re.search(r'extern "C" [\w\s\*]*k##%s\(' % sfx, header), sfx
    builds = re.search(r"#define DT_TRACE_BUILDS\(X\)(.*?)\n#define", header, re.S).group(1)
    assert len(re.findall(r"X\((dt_trace_kernel\w*)\)", builds)) == 14
    assert "DT_TRACE_DECL(k) DT_TRACE_DECL(k##_win) DT_TRACE_DECL(k##_awin)" in header
