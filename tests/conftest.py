"""pytest configuration: repo root on sys.path, the `gpu` marker, shared fixtures."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The reference's data fixtures (SGF games, minimodel.json, Keras HDF5 files) are stored under
# tests/golden/reference in the reference's own layout (minimodel.json and the dataset's file
# offsets name paths from its root), so the compatibility tests run from the repository alone.
REFERENCE_DATA = os.path.join(ROOT, "tests", "golden", "reference", "tests", "test_data")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP kernels, RCCL)")
    config.addinivalue_line("markers", "slow: long-running test")


@pytest.fixture
def ref_data():
    assert os.path.isdir(REFERENCE_DATA), REFERENCE_DATA + " is missing"
    return REFERENCE_DATA


@pytest.fixture
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")
