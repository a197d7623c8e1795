"""fdc_sinks_set_payload_format and friends: what can be checked without a device — the exported symbols and their declared signatures, the
argument checks that come before anything touches a device, and the format names the Python faces take."""
import ctypes as C
import os
import re

import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd import sinks as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fdc_amd.h")
DECLARED = {
    "fdc_sinks_set_payload_format": ("int", "fdc_sinks *s, int32_t format, float scale", (C.c_int, [C.c_void_p, C.c_int32, C.c_float])),
    "fdc_sinks_payload_format": ("int", "const fdc_sinks *s, int32_t *format, float *scale",
                                 (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)])),
    "fdc_sinks_payload_route": ("int32_t", "const fdc_sinks *s", (C.c_int32, [C.c_void_p])),
    "fdc_sinks_group_set_payload_format": ("int", "fdc_sinks_group *g, int32_t format, float scale", (C.c_int, [C.c_void_p, C.c_int32, C.c_float])),
}


def test_new_symbols_are_exported_with_the_declared_signatures():
    text = open(HEADER).read()
    lib = G.lib()
    for name, (ret, args, binding) in DECLARED.items():
        m = re.search(r"^(\w+) %s\(([^)]*)\);" % name, text, re.M)
        assert m, name
        assert m.group(1) == ret and re.sub(r"\s+", " ", m.group(2)).strip() == args, (name, m.groups())
        assert _lib.SYMBOLS[name] == binding, name
        assert getattr(lib, name) is not None
    assert (_lib.FDC_OQ_FC32, _lib.FDC_OQ_SC16, _lib.FDC_OQ_SC8) == (0, 1, 2)
    assert "complex float32, owned by the handle" not in text       # the struct comment names the payload format now


def test_entry_points_validate_without_a_device():
    """Null handles and null out-pointers are refused before anything touches a device (and fdc_last_error says so)."""
    lib = G.lib()
    f, sc = C.c_int32(7), C.c_float(7.0)
    assert lib.fdc_sinks_set_payload_format(None, _lib.FDC_OQ_SC16, 1.0) == -1 and b"null" in lib.fdc_last_error()
    assert lib.fdc_sinks_payload_format(None, C.byref(f), C.byref(sc)) == -1 and b"null" in lib.fdc_last_error()
    assert (f.value, sc.value) == (7, 7.0)
    assert lib.fdc_sinks_payload_route(None) == -1
    assert lib.fdc_sinks_group_set_payload_format(None, _lib.FDC_OQ_SC8, 1.0) == -1 and b"null" in lib.fdc_last_error()
    # null out-pointers: refused before the handle is looked at (any non-null address will do here)
    dummy = C.create_string_buffer(64)
    assert lib.fdc_sinks_payload_format(C.addressof(dummy), None, C.byref(sc)) == -1 and b"null" in lib.fdc_last_error()
    assert lib.fdc_sinks_payload_format(C.addressof(dummy), C.byref(f), None) == -1
    assert (f.value, sc.value) == (7, 7.0)


def test_python_faces_reject_unknown_format_names():
    assert [S.payload_format_code(n) for n in (None, "fc32", "sc16", "SC8")] == [0, 0, 1, 2]
    for bad in ("sc12", "int16", "", 1, 2.0, b"sc16"):
        with pytest.raises(ValueError):
            S.payload_format_code(bad)
    # the faces check the name (and the verbose modes, which decide on the host) before they create anything on a device
    with pytest.raises(ValueError):
        G.PowerActivationChannel(4096, 0.3, 0.05, 2, 6.0, -1, 0, True, False, "", 0, 1, payload_format="ci16")
    with pytest.raises(ValueError):
        G.PowerActivationChannel(4096, 0.3, 0.05, 2, 6.0, -1, 0, True, False, "", 1, 1, payload_format="sc16")
    with pytest.raises(ValueError):
        G.activity_detection_channelizer_vcm(4096, [(0.1, 0.4)], 10.0, 2, -1, True, False, "", False, 0.005, 1, 0.2, 0, payload_format="s16")
    with pytest.raises(ValueError):
        G.SegmentDetection(0, 4096, 2, 0.1, 0.4, 10.0, 0.005, 0.2, -1, 1, True, False, "", False, 2, payload_format="sc8")
    with pytest.raises(ValueError):
        G.FrequencyDomainChannelizer(8, 1, 4096, 2, [[0.1, 0.05]], [[-0.2, 0.04]], 6.0, 1.0, 0.0, 'normalized', 1, True, False, "", False,
                                     [[0.25, 0.4]], 10.0, 0.005, 1, 0.2, 0, 0, 3, 3, False, payload_format="sc24")
    with pytest.raises(TypeError):                                  # keyword-only
        G.PowerActivationChannel(4096, 0.3, 0.05, 2, 6.0, -1, 0, True, False, "", 0, 1, 0, 64, "sc16")
