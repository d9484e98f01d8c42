import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    # (split fixtures -- parts, triangle-stored matrices -- come back merged: oracle/golden.py)
    from oracle.golden import load as load_golden

    def load(name):
        return load_golden(name, GOLDEN)
    return load
