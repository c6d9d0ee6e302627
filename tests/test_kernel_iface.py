"""The host/kernel boundary is declared once (distraytracer_amd/csrc/dt_kernel_iface.h): dt_kernels.hip includes
the header, so a definition that disagrees with its declaration does not compile; the two host units declare
none of its symbols themselves; and every such extern "C" function the kernels' file defines is in the header.
Plain regular expressions over the sources. No GPU."""
import os
import re

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


def test_every_interface_function_the_kernels_define_is_declared_in_the_header():
    hip, header = read("dt_kernels.hip"), read("dt_kernel_iface.h")
    assert re.search(r'^#include "dt_kernel_iface.h"$', hip, re.M)
    assert not re.search(r"^#if", hip[:hip.index('#include "dt_kernel_iface.h"')], re.M), "included in every build"
    declared = extern_c_names(header)
    defined = {n for n in extern_c_names(hip) if IFACE.match(n)}
    assert len(defined) >= 30
    assert sorted(defined - declared) == []
    # the trace builds' trio is defined through DT_CAT(DT_TRACE_KERNEL, _launch | _ptr | _traits), DT_TRACE_KERNEL
    # being the build's kernel name (the Makefile's -DDT_KNAME, DT_WINDOW's _win / _awin): the header declares the
    # trio for every name of its list in all three modes
    for sfx in ("_launch", "_ptr", "_traits"):
        assert re.search(r'extern "C" [\w\s\*]*DT_CAT\(DT_TRACE_KERNEL, %s\)' % sfx, hip), sfx
        assert re.search(r'extern "C" [\w\s\*]*k##%s\(' % sfx, header), sfx
    builds = re.search(r"#define DT_TRACE_BUILDS\(X\)(.*?)\n#define", header, re.S).group(1)
    assert len(re.findall(r"X\((dt_trace_kernel\w*)\)", builds)) == 14
    assert "DT_TRACE_DECL(k) DT_TRACE_DECL(k##_win) DT_TRACE_DECL(k##_awin)" in header
