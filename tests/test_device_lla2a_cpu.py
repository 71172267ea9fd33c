"""CPU tests of ncclLLA2ASession's header (include/nccl_device_ll_a2a.h): the stand-alone host sweep of the requirement,
slot and epoch functions (built under ASan+UBSan), and the test kernels and the example cross-compiled for gfx950."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_sweep(built):
    subprocess.check_call(["make", "-s", "devapi-lla2a-host-test"], cwd=ROOT)
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "devapi_lla2a_host_test")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_kernels_compile_for_gfx950(built):
    subprocess.check_call(["make", "-s", "devapi-lla2a-kernels", "devapi-lla2a-example"], cwd=ROOT)
    assert os.path.exists(os.path.join(ROOT, "tests", "native", "libdevapi_lla2a_kernels.so"))
