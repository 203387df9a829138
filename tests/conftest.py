import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REFERENCE = "/root/reference"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def have_reference():
    return os.path.isdir(os.path.join(REFERENCE, "Src", "Speech_Recog"))


needs_reference = pytest.mark.skipif(not have_reference(), reason="/root/reference not present (GPU box)")


def have_ref_objects():
    """the reference's own objects, compiled by build() into oracle/_ref/ where the reference tree exists (they travel with
    the working tree to where it does not)"""
    return have_reference() or all(os.path.exists(os.path.join(ROOT, "oracle", "_ref", f))
                                   for f in ("libsr_ref.so", "libsr_ref320.so"))


needs_ref_objects = pytest.mark.skipif(not have_ref_objects(), reason="oracle/_ref/ not built: no reference tree at build time")
