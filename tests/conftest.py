import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a HIP device (MI355X); run with -m gpu on the GPU box")
    config.addinivalue_line("markers", "slow: long-running test")


@pytest.fixture(autouse=True)
def _fresh_process_context():
    """The single-process context (runtime/comm.py) is created once and then reused: a test that
    launches with ``cpu=True`` would leave a CPU context behind, and a later test in the same
    process that launches on the GPU would get CPU-resident weights next to device-resident data.
    Every test starts without one.  (Spawned ranks own their process groups and are not touched.)"""
    yield
    comm = sys.modules.get("rocket_amd.runtime.comm")
    if comm is not None and comm._CTX is not None and not comm._CTX.distributed:
        comm._CTX = None


def pytest_collection_modifyitems(config, items):
    import torch

    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no HIP device")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
