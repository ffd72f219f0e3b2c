"""The shared test helpers themselves (tests/gpu_support.py and its neighbours)."""
import ast
import glob
import os

import numpy as np

import noise_aead
from gpu_support import REC_DT
from host_check import ROOT


def test_rec_dt_is_the_record_the_library_reads():
    """The one literal record dtype against the ctypes mirror of NoiseAeadRecord:
    names, formats and offsets of every field, and the 48-byte item size."""
    mirror, dt = np.dtype(noise_aead.NoiseAeadRecord), np.dtype(REC_DT)
    assert dt == mirror
    assert dt.names == mirror.names == tuple(n for n, _ in noise_aead.NoiseAeadRecord._fields_)
    assert [dt.fields[n] for n in dt.names] == [mirror.fields[n] for n in dt.names]
    assert dt.itemsize == mirror.itemsize == 48


def test_no_file_imports_a_test_module():
    """A helper that two files use lives in a plain module: nothing under
    tests/ or tools/ imports a module named test_*."""
    files = glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True)
    files += glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)
    assert len(files) > 80
    found = []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                [node.module or ""] + [a.name for a in node.names] if isinstance(node, ast.ImportFrom) else []
            found += [(os.path.relpath(path, ROOT), node.lineno, n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not found, found
