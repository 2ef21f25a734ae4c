"""GPU: the sibling reductions of the host mirror (csrc/host/EnsembleCalculators) over fields registered in their native
formats -- the members go to the device as they are stored and the fields equal the oracle on the converted values."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from correrender_amd import engine, synth
from parity import assert_bit_exact

ROOT = Path(__file__).resolve().parent.parent
ENSEMBLE_EXE = ROOT / "correrender_amd" / "ensemble_formats_host_test"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["u8", "u16", "f16", "f32"])
def test_reduce_calculators_fed_native_fields_upload_natively(tmp_path, oracle, fmt):
    xs, ys, zs, cs = 13, 11, 7, 24
    ens = synth.box_ensemble(xs, ys, zs, cs, seed=22)
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
    r = subprocess.run([str(ENSEMBLE_EXE), str(tmp_path / "in.bin"), str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "ENSEMBLE-OK" in r.stdout, r.stdout + r.stderr
    assert f"RESIDENT-FORMAT {code}\n" in r.stdout, r.stdout
    read = lambda name: np.fromfile(tmp_path / name, np.float32)
    assert_bit_exact(read("mean.bin"), oracle.ensemble_stat(0, wide), f"mean calculator on {fmt} fields")
    assert_bit_exact(read("spread.bin"), oracle.ensemble_stat(1, wide), f"spread calculator on {fmt} fields")
    # the program's settings: members > 0.5, counts 2..20
    assert_bit_exact(read("predicate.bin"), oracle.set_predicate(0, 0.5, 2, 20, wide), f"predicate calculator on {fmt} fields")
