import os
import sys

import pytest
# torch before anything can load librustybam_amd.so: torch brings its own copy of the HIP runtime, and whichever copy is loaded first
# serves the whole process.  With the library (linked against the system's copy) loaded first -- tests/test_capi_load.py does, and in a
# run of the whole suite it comes before the GPU tests -- a later torch.cuda initialisation loads the second copy and the engine finds
# no device.
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (gfx950); run with -m gpu on the GPU box")


@pytest.fixture(scope="session")
def golden():
    return GOLDEN


@pytest.fixture(scope="session")
def oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="session")
def engine():
    """The product library on cuda:0.  No fallback: a missing library or device is a test ERROR."""
    # (torch is already loaded, at the top of this file: tests/test_gpu_fullsize.py and others use it for device memory beside the engine)
    import rustybam_amd
    eng = rustybam_amd.Engine(0)
    yield eng
    eng.close()
