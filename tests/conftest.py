import os
import sys

import pytest

# the GPU tests run with the hardware-queue count bench.py uses (streams on separate queues really
# run concurrently: this is what exposed the missing side-stream wait of synchronous bucketed
# clocks); set before anything imports torch
if os.environ.get("GPU_MAX_HW_QUEUES", "4") == "4":  # unset or HIP's default (the GPU box exports 4)
    os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("MINIPS_HW_QUEUES", "8")

# the launcher's pid files (minips_amd/launch.py) go to a directory of this test session, not to
# the fixed per-machine default, which another user's run may have left behind unwritable; set
# before minips_amd.launch is imported, inherited by the processes the tests start
if "MINIPS_PID_DIR" not in os.environ:
    import atexit
    import shutil
    import tempfile

    os.environ["MINIPS_PID_DIR"] = tempfile.mkdtemp(prefix="minips_pids_")
    atexit.register(lambda d=os.environ["MINIPS_PID_DIR"], pid=os.getpid():
                    os.getpid() == pid and shutil.rmtree(d, ignore_errors=True))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP) device")


def gpu_available():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)
