"""GPU: the SEPARATE_SYMMETRIC mode of the host mirror (csrc/host/CorrelationCalculator) over two fields registered in their
native formats -- both fields go to the device as they are stored and the Pearson field equals the oracle on the converted
values."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from correrender_amd import engine, synth
from parity import assert_bit_exact
import oracle_lib

ROOT = Path(__file__).resolve().parent.parent
SECONDARY_EXE = ROOT / "correrender_amd" / "secondary_formats_host_test"


def _field(xs, ys, zs, cs, seed, fmt):
    ens = synth.box_ensemble(xs, ys, zs, cs, seed=seed)
    ens = ((ens - ens.min()) / (ens.max() - ens.min())).astype(np.float32)
    if fmt == "u16":
        narrow = np.rint(ens * np.float32(65535)).astype(np.uint16)
        return narrow, narrow.astype(np.float32) / np.float32(65535)
    if fmt == "u8":
        narrow = np.rint(ens * np.float32(255)).astype(np.uint8)
        return narrow, narrow.astype(np.float32) / np.float32(255)
    if fmt == "f16":
        narrow = ens.astype(np.float16)
        return narrow, narrow.astype(np.float32)
    return ens, ens


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["u8", "u16", "f16", "f32"])
def test_symmetric_mode_fed_native_fields_uploads_both_natively(tmp_path, oracle, fmt):
    xs, ys, zs, cs = 13, 11, 7, 24
    first, wide_first = _field(xs, ys, zs, cs, 22, fmt)
    second, wide_second = _field(xs, ys, zs, cs, 23, fmt)
    code = engine.MEMBER_FORMATS.index(fmt)
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([xs, ys, zs, cs, code], np.int32).tofile(f)
        np.ascontiguousarray(first).tofile(f)
        np.ascontiguousarray(second).tofile(f)
    r = subprocess.run([str(SECONDARY_EXE), str(tmp_path / "in.bin"), str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "SECONDARY-OK" in r.stdout, r.stdout + r.stderr
    assert f"RESIDENT-FORMAT {code}\n" in r.stdout, r.stdout
    assert f"RESIDENT-SECONDARY-FORMAT {code}\n" in r.stdout, r.stdout
    got = np.fromfile(tmp_path / "symmetric.bin", np.float32)
    assert_bit_exact(got, oracle.symmetric_field(oracle_lib.PEARSON, wide_first, wide_second), f"symmetric pearson on {fmt} fields")
