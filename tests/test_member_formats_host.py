"""CPU: the narrow member formats at the ABI boundary -- the header stays plain C99 with the new declarations, the python
binding table binds them, and without a GPU nothing is computed."""
import ctypes
import subprocess

import pytest
from pathlib import Path

import correrender_amd as ca
from correrender_amd import _lib, engine

ROOT = Path(__file__).resolve().parent.parent

NEW_SYMBOLS = ["crf_upload_members_format", "crf_bind_members_device_format", "crf_member_format", "crf_last_member_format"]


def test_header_with_member_formats_is_plain_c(tmp_path):
    src = tmp_path / "formats.c"
    src.write_text('#include "corrfield.h"\n'
                   'int main(void){ enum crf_member_format f = CRF_MEMBER_F16;\n'
                   '  int (*up)(crf_context*, int, const void* const*) = crf_upload_members_format;\n'
                   '  int (*bind)(crf_context*, int, const void* const*) = crf_bind_members_device_format;\n'
                   '  int (*get)(const crf_context*) = crf_member_format;\n'
                   '  int (*last)(const crf_context*) = crf_last_member_format;\n'
                   '  return (up && bind && get && last) ? (int)f + CRF_MEMBER_F32 + CRF_MEMBER_U8 + CRF_MEMBER_U16 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "formats.o")], check=True)


def test_binding_table_has_the_format_symbols():
    lib = ca.load_library()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    assert lib.crf_abi_version() == 5
    # a null context: F32, and an argument error that touches no device
    assert lib.crf_member_format(None) == 0 and lib.crf_last_member_format(None) == 0
    assert lib.crf_upload_members_format(None, 2, (ctypes.c_void_p * 1)(1)) == 1


def test_dtype_to_format():
    import numpy as np
    import torch
    assert [engine._member_format(d) for d in (np.dtype(np.float32), np.dtype(np.uint8), np.dtype(np.uint16),
                                               np.dtype(np.float16))] == [0, 1, 2, 3]
    assert [engine._member_format(d) for d in (torch.float32, torch.uint8, torch.uint16, torch.float16)] == [0, 1, 2, 3]
    assert engine.MEMBER_FORMATS == ["f32", "u8", "u16", "f16"]
    for bad in (np.dtype(np.float64), np.dtype(np.int16), torch.bfloat16, torch.int8):
        try:
            engine._member_format(bad)
        except TypeError:
            continue
        raise AssertionError(f"{bad} accepted")


# ---- the host mirror (csrc/host/VolumeData.hpp: ScalarDataFormat, HostCacheEntryType) -------------------------------------
FORMAT_EXE = ROOT / "correrender_amd" / "member_formats_host_test"


def _rounding_probes():
    """Floats whose float16 rounding is decided in every possible way: every finite half, the midpoint between every two
    neighbours (a tie) and the floats next to it on both sides; the same around the largest half (overflow to infinity
    at 65520) and below the smallest denormal; +-0, +-Inf."""
    import numpy as np
    bits = np.arange(65536, dtype=np.uint32)
    halves = bits[(bits & 0x7C00) != 0x7C00].astype(np.uint16).view(np.float16).astype(np.float32)
    pos = np.sort(halves[halves >= 0])
    mid = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2).astype(np.float32)  # exact: one more bit
    extra = np.array([65519.996, 65520.0, 65520.004, 65536.0, 1e9, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), 1),
                      2.0 ** -26, 1e-30, np.inf], np.float32)
    mag = np.concatenate([pos, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)), extra])
    return np.concatenate([mag, -mag]).astype(np.float32)


def test_host_mirror_conversions_match_numpy_for_every_code(tmp_path):
    import numpy as np
    probes = _rounding_probes()
    probes.tofile(tmp_path / "floats.bin")
    r = subprocess.run([str(FORMAT_EXE), "convert", str(tmp_path / "floats.bin"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "CONVERT-OK" in r.stdout, r.stdout + r.stderr
    same = lambda a, b: (a.view(np.uint32) == b.view(np.uint32)).all()
    u8 = np.fromfile(tmp_path / "u8.bin", np.float32)
    assert u8.size == 256 and same(u8, np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255))
    u16 = np.fromfile(tmp_path / "u16.bin", np.float32)
    assert u16.size == 65536 and same(u16, np.arange(65536).astype(np.uint16).astype(np.float32) / np.float32(65535))
    f16 = np.fromfile(tmp_path / "f16.bin", np.float32)
    codes = np.arange(65536).astype(np.uint16)
    finite = (codes & 0x7C00) != 0x7C00
    want = codes.view(np.float16).astype(np.float32)
    assert finite.sum() == 63488 and same(f16[finite], want[finite])
    assert (np.isnan(f16[~finite]) == np.isnan(want[~finite])).all() and same(f16[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)])
    # switchNativeFormat(FLOAT16): round to nearest even
    half = np.fromfile(tmp_path / "half.bin", np.uint16)
    with np.errstate(over="ignore"):
        want_half = probes.astype(np.float16).view(np.uint16)
    assert half.size == probes.size
    bad = np.nonzero(half != want_half)[0]
    assert bad.size == 0, [(float(probes[i]), hex(half[i]), hex(want_half[i])) for i in bad[:5]]
    assert np.unique(half).size == 63488 + 2  # every finite half and both infinities are produced


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["u16", "u8", "f16", "f32"])
def test_calculator_fed_native_fields_uploads_natively(tmp_path, oracle, fmt):
    """A CorrelationCalculator over fields registered with setFieldData(format) keeps the members resident in that format
    (crf_upload_members_format) and its Pearson field equals the oracle on the converted values; float fields stay f32."""
    import numpy as np
    import oracle_lib
    from correrender_amd import synth
    from parity import assert_bit_exact
    xs, ys, zs, cs = 13, 11, 7, 24
    ens = synth.box_ensemble(xs, ys, zs, cs, seed=21)
    ens = ((ens - ens.min()) / (ens.max() - ens.min())).astype(np.float32)
    if fmt == "u16":
        narrow = np.rint(ens * np.float32(65535)).astype(np.uint16)
        wide = narrow.astype(np.float32) / np.float32(65535)
    elif fmt == "u8":
        narrow = np.rint(ens * np.float32(255)).astype(np.uint8)
        wide = narrow.astype(np.float32) / np.float32(255)
    elif fmt == "f16":
        narrow = ens.astype(np.float16)
        wide = narrow.astype(np.float32)
    else:
        narrow = wide = ens
    code = engine.MEMBER_FORMATS.index(fmt)
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([xs, ys, zs, cs, code], np.int32).tofile(f)
        np.ascontiguousarray(narrow).tofile(f)
    r = subprocess.run([str(FORMAT_EXE), "upload", str(tmp_path / "in.bin"), str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "UPLOAD-OK" in r.stdout, r.stdout + r.stderr
    assert f"RESIDENT-FORMAT {code}\n" in r.stdout, r.stdout
    got = np.fromfile(tmp_path / "pearson.bin", np.float32)
    ref = wide[:, zs // 2, ys // 2, xs // 2].copy()  # the calculator's default reference point: the grid centre
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, wide, ref), f"calculator on {fmt} fields")
