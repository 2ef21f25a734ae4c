"""CPU: crf_wide_copy_bytes at the ABI boundary -- the header stays plain C99 with the new declaration, the python binding
table binds it with the header's types, and a null context holds no copy."""
import ctypes
import subprocess
from pathlib import Path

import correrender_amd as ca
from correrender_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_header_with_wide_copy_bytes_is_plain_c(tmp_path):
    src = tmp_path / "wide.c"
    src.write_text('#include "corrfield.h"\n'
                   'int main(void){ size_t (*f)(const crf_context*) = crf_wide_copy_bytes;\n'
                   '  return f ? crf_abi_version() - crf_abi_version() : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "wide.o")], check=True)


def test_binding_table_has_wide_copy_bytes():
    assert _lib.SYMBOLS["crf_wide_copy_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p])
    lib = ca.load_library()
    assert lib.crf_wide_copy_bytes.restype is ctypes.c_size_t
    assert lib.crf_wide_copy_bytes.argtypes == [ctypes.c_void_p]
    assert lib.crf_abi_version() == 5


def test_null_context_holds_no_copy():
    assert ca.load_library().crf_wide_copy_bytes(None) == 0


def test_engine_exposes_wide_copy_bytes():
    assert callable(ca.CorrField.wide_copy_bytes)


def test_header_names_the_function_among_the_compatible_additions():
    header = (ROOT / "include" / "corrfield.h").read_text()
    version = header[header.index("int crf_abi_version(void);"):]
    assert "crf_wide_copy_bytes" in version[:version.index("4: crf_group_")]
