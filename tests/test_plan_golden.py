"""CPU test that host planning computes what it computed when tests/golden/plan_digest.txt was recorded (no GPU).

tests/native/plan_test `sweep` plans a grid of collectives and groups in process, with the launches stubbed, and
prints per (configuration, rank count) the number of cases and, per collective, a 64-bit FNV-1a hash of every member
of every launch argument block they produced (LaunchPlan, CollArgs, LLBatchArgs, CollBatchArgs, SymPlan, SymArgs,
SymA2AArgs), of what planning passed to the window, registration and tuner lookups, the result code and the op
counter. Every rank must derive the same plan from the same inputs, so a
change of the planning code that is meant to keep plans as they are must leave every line as it is. Where a line
differs, `plan_test sweep-full` of the two builds prints the dumps themselves, to be diffed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "plan_test")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digest.txt")


def test_plan_digest_matches_golden():
    subprocess.check_call(["make", "plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    # the sweep sets and unsets the variables it sweeps itself; nothing else of the caller's may reach the planner
    env = {k: v for k, v in os.environ.items() if not k.startswith(("NCCL_", "PLAN_"))}
    env["NCCL_CONF_FILE"] = os.devnull
    env["HOME"] = os.path.join(ROOT, "tests", "golden")  # (no ~/.nccl.conf there)
    out = subprocess.run([EXE, "sweep"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = out.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(want) > 300
    differing = [(w, g) for w, g in zip(want, got) if w != g]
    assert not differing, "%d of %d digest lines differ; the first: golden %r, this build %r" % (
        len(differing), len(want), differing[0][0], differing[0][1])
    assert len(got) == len(want)
