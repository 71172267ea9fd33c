"""CPU tests of the device API's reduce-copy addition (include/nccl_device.h ncclSymPtr,
include/nccl_device_reduce_copy.h): the stand-alone host sweep of ncclSymPtr and of the plan function (built under
ASan+UBSan), the gfx950 code of the test kernels (16-byte accesses in the float ncclLsaReduceSumCopy kernel, no scratch
and no spill in any kernel), the edge-value input sets and numpy reference of tests/test_gpu_device_rc_edge.py (NaN
cap, one-NaN results, and that the sets tell a wrong fold from the right one), and the header as a host-only C++17
translation unit."""
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


def test_edge_sets_discriminate(built):
    """The inputs and the reference of tests/test_gpu_device_rc_edge.py, without a GPU: every set's reference result
    stays under the NaN cap at every nSrc; an element with exactly one NaN among its sources (and none made by the
    fold) results in that input's bits; and the sets tell a wrong fold from the right one — on `dr` a fold that rounds
    per step differs from the fp32 fold on at least 40 % of the non-NaN elements, on `order` the fold with the last two
    sources exchanged on at least 10 %, on `many` the reversed fold on at least 1 % at every nSrc."""
    import numpy as np
    from tests import gpu_cases as G
    from tests import test_gpu_device_rc_edge as E
    for kind in E.KINDS:
        sets = E.edge_sets(kind)
        assert set(sets) == ({"edge", "many"} | ({"dr", "dr1", "order", "many17"} if kind in E.SHORT else set()))
        for name, (srcs, nsrcs) in sets.items():
            ref = E.ref_sum(kind, srcs, nsrcs)
            for nsrc in nsrcs:
                want, one = ref[nsrc]
                share = E.nan_share(kind, want)
                exact = float((~np.isnan(E.up(kind, want)) | one).mean())
                print(f"[{kind} {name} nSrc={nsrc}] NaN share {100 * share:.2f} %, compared bit for bit "
                      f"{100 * exact:.2f} %")
                assert share <= E.NAN_CAP and G.nan_cap_ok(want, E.KINDS[kind]), (kind, name, nsrc, share)
                assert one.any() or name not in ("edge", "many", "many17")
                nans = np.stack([np.isnan(E.up(kind, s)) for s in srcs[:nsrc]])
                theirs = np.stack([G._raw(s) for s in srcs[:nsrc]])[nans.argmax(0), np.arange(want.size)]
                assert np.array_equal(G._raw(want)[one], theirs[one]), (kind, name, nsrc)
            if name in ("edge", "dr", "dr1", "order"):
                for op in ("sum", "max"):
                    want, one = E.ref_fold_T(kind, srcs, op)
                    assert E.nan_share(kind, want) <= E.NAN_CAP, (kind, name, op)
                    if op == "sum":
                        nans = np.stack([np.isnan(E.up(kind, s)) for s in srcs])
                        theirs = np.stack([G._raw(s) for s in srcs])[nans.argmax(0), np.arange(want.size)]
                        assert np.array_equal(G._raw(want)[one], theirs[one]), (kind, name, op)
        many = sets["many"][0]
        for nsrc in E.MANY_NSRC:
            fwd = E.ref_sum(kind, many[:nsrc])[nsrc][0]
            rev = E.ref_sum(kind, many[:nsrc][::-1])[nsrc][0]
            share = E.differing_share(kind, fwd, rev)
            print(f"[{kind} many nSrc={nsrc}] the reversed fold differs on {100 * share:.1f} %")
            assert share >= 0.01, (kind, nsrc, share)
        if kind not in E.SHORT:
            continue
        for name in ("dr", "dr1"):
            srcs = sets[name][0]
            share = E.differing_share(kind, E.ref_fold_T(kind, srcs, "sum")[0], E.ref_sum(kind, srcs)[3][0])
            print(f"[{kind} {name}] the per-step fold in T differs from the fp32 fold on {100 * share:.1f} %")
            assert name != "dr" or share >= 0.40, (kind, name, share)
        a, swapped, nega = sets["order"][0]
        share = E.differing_share(kind, E.ref_sum(kind, [a, nega, swapped])[3][0],
                                  E.ref_sum(kind, [a, swapped, nega])[3][0])
        print(f"[{kind} order] [a, -a, swapped] differs from [a, swapped, -a] on {100 * share:.1f} %")
        assert share >= 0.10, (kind, share)
    # the reference's bf16 rounding on its own: ties to even, a carry into the exponent, overflow to Inf, a quiet NaN
    f = np.array([0x3f808000, 0x3f818000, 0x3f7f8000, 0x7f7f8000, 0x7f800001, 0xffc12345, 0x00008000, 0x00018000],
                 dtype=np.uint32).view(np.float32)
    assert E.down("bfloat16", f).tolist() == [0x3f80, 0x3f82, 0x3f80, 0x7f80, 0x7fc0, 0xffc1, 0x0000, 0x0002]


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
