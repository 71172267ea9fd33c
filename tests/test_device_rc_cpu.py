"""CPU tests of the device API's reduce-copy addition (include/nccl_device.h ncclSymPtr,
include/nccl_device_reduce_copy.h): the stand-alone host sweep of ncclSymPtr and of the plan function (built under
ASan+UBSan), the gfx950 code of the test kernels (16-byte accesses in the float ncclLsaReduceSumCopy kernel, no scratch
and no spill in any kernel), and the header as a host-only C++17 translation unit."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
RCBUILD = os.path.join(ROOT, "build", "devapi_rc")


def test_symptr_and_plan_host_sweep(built):
    """tests/native/devapi_rc_host_test: ncclSymPtr on a fake window table (construction, conversion, element-counted
    steps of the six integer types with negative steps, differences, comparisons) and ncclReduceCopyPlan for every
    element size, every source / destination low-address pattern mod 16 and every count 0..200 plus large ones: the
    segments tile [0, count) in order, 16-byte segments start 16-byte aligned on all pointers, 4-byte segments 4-byte
    aligned, and the prefix is shorter than one pack."""
    subprocess.check_call(["make", "-s", "devapi-rc-host-test"], cwd=ROOT)
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "devapi_rc_host_test")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert int(re.search(r"plans=(\d+)", r.stdout).group(1)) > 100000


def _kernel_build():
    """The test kernels' assembly and resource-usage remarks, which `make devapi-rc-kernels` leaves in build/devapi_rc."""
    subprocess.check_call(["make", "-s", "devapi-rc-kernels"], cwd=ROOT)
    asm = open(os.path.join(RCBUILD, "devapi_rc_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    usage = open(os.path.join(RCBUILD, "kernels.usage")).read()
    return asm, usage


def test_float_reduce_sum_copy_moves_16_bytes(built):
    """The float LSA kernel (every ncclLsaReduceSumCopy overload on float) loads and stores 16 bytes per lane, and its
    unchecked round issues the four loads of a source back to back."""
    asm, _ = _kernel_build()
    m = re.search(r"^(_Z11rcLsaKernelIfEv\w*):\s.*?s_endpgm", asm, re.M | re.S)
    assert m, "the float LSA kernel is not in the assembly"
    body = m.group(0)
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
    lines = body.splitlines()
    at = [i for i, line in enumerate(lines) if "global_load_dwordx4" in line]
    assert any(b - a <= 8 for a, b in zip(at, at[3:])), "no four 16-byte loads issued together"


def test_no_kernel_uses_scratch_or_spills(built):
    _, usage = _kernel_build()
    names = re.findall(r"Function Name: (\S+)", usage)
    assert len(names) >= 60 and any(n.startswith("_Z11rcLsaKernelIfE") for n in names), names[:5]
    fields = {f: [int(v) for v in re.findall(rf"{f}: (\d+)", usage)]
              for f in (r"ScratchSize \[bytes/lane\]", "SGPRs Spill", "VGPRs Spill")}
    for f, vals in fields.items():
        assert len(vals) == len(names), f
        bad = [(n, v) for n, v in zip(names, vals) if v]
        assert not bad, f"{f}: {bad[:10]}"


def test_header_compiles_host_only(tmp_path):
    """Without hipcc: the types, ncclSymPtr and the plan function are there; the device functions are not."""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    ok = tmp_path / "host_only.cc"
    ok.write_text('#include "nccl_device.h"\n'
                  "ncclSymPtr<float> f(ncclWindow_t w) { return ncclSymPtr<float>(w, 16) + 3; }\n"
                  "size_t g() { return ncclReduceCopyPlan(4, 0, 4, 100).prefix + ncclReduceCopyRoundElts(4, 256, 16); }\n"
                  "static_assert(sizeof(ncclSymPtr<double>) == 16, \"\");\n")
    r = subprocess.run([CLANGXX, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *inc, str(ok)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for use in ("ncclSymPtr<float>().localPtr()", "ncclLsaCopy<float>(0, (float*)0, ncclSymPtr<float>(), 0, ncclTeam())",
                "ncclCoopCta()"):
        bad = tmp_path / "device_use.cc"
        bad.write_text('#include "nccl_device.h"\n' f"void f() {{ (void){use}; }}\n")
        r = subprocess.run([CLANGXX, "-std=c++17", "-fsyntax-only", *inc, str(bad)], capture_output=True, text=True)
        assert r.returncode != 0, f"{use} compiled in a host-only translation unit"
