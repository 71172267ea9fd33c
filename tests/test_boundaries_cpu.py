"""CPU tests of the boundary-count generator and the guarded arenas of tests/gpu_cases.py (no GPU).

1. The generator hits what it claims. For every path of gpu_cases.BOUNDARY_ENVS, collective, n in {2, 3} and element
   size in {1, 2, 4, 8}, every generated count is planned by tests/native/plan_test under the path's environment
   (its `many` form: one process per (path, n) plans every count; PLAN_GEOMETRY=1 gives the communicator the shape
   init.cc reads from that environment, PLAN_WINDOW=1 puts the buffers in a symmetric window). From the printed plan
   the classes of each count are recomputed (gpu_cases.classify over the real plans) and must contain the claimed
   ones; every class gpu_cases.reachable_classes lists must be hit; the model's plan must equal the real one field by
   field; the invariants of test_planning.py::test_plan_invariants must hold at every count; and the planned kernel
   must be the path's, the counts built to leave it included.
2. The arena comparison (gpu_cases.arena_errors) reports planted faults: a numpy mock collective writes the oracle's
   results into the arena images, then one fault at a time is planted and must be reported with its rank and count.
3. classify itself is pinned at counts whose plan and classes were worked out by hand (ANCHORS), and the eight counts
   the GPU test issues in one group are planned as one staged launch whose channel ranges wrap the cap.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import gpu_cases as G
from tests.test_planning import EXE, ROOT, plan

NS = (2, 3)
SIZES = (1, 2, 4, 8)
PLAN_KEYS = ("algo", "nch", "part", "slice", "steps", "chunk", "cbdlo", "cbdhi", "refnch", "sub", "kind", "symcoll")
# the kernel family plan_test names for each path's own plans
PATH_ALGO = {"DIRECT": {"direct"}, "PULLS_AG0": {"direct"}, "PULLS_AG1": {"direct"}, "ONESHOT": {"oneshot"},
             "LL": {"ll"}, "LL128": {"ll128"}, "TREE": {"chain"}, "REF_ORDER": {"direct"}, "REF_SUB": {"direct"},
             "WINDOW": {"sym"}, "WINDOW_ONESHOT": {"sym"}, "TABLE": {"ll", "ll128", "oneshot", "direct"}}
# where a count built to leave an LL path goes (the default algorithm: one-shot AllReduce up to 2 MiB / n, else direct)
LL_FALLBACK = {"allreduce": "oneshot", "reducescatter": "direct", "allgather": "direct", "reduce": "direct"}


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "native", "plan_test.cc")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(src):
        subprocess.check_call(["make", "plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    return EXE


def path_env(path):
    env = dict(G.BOUNDARY_ENVS[path], PLAN_GEOMETRY="1")
    if path in G.BOUNDARY_WINDOW_PATHS:
        env["PLAN_WINDOW"] = "1"
    return env


def plan_many(exe, path, n, specs):
    """The plans of [(collective, element size, call count), ...] on one communicator of n ranks under the path's
    environment: one plan_test process."""
    e = {k: v for k, v in os.environ.items() if not k.startswith(("NCCL_", "PLAN_"))}
    e.update(path_env(path))
    args = [f"{G._PLAN_FUNC[coll]}:{G._DTYPE_OF_SIZE[es]}:{c}" for coll, es, c in specs]
    out = subprocess.run([exe, str(n), "many", *args], env=e, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.split("\n") if ln.startswith(("algo=", "error="))]
    assert len(lines) == len(specs), (len(lines), len(specs))
    return [{k: (v if k == "algo" else int(v)) for k, v in (t.split("=") for t in ln.split())} for ln in lines]


_real: dict = {}


def real_plans(exe, path, n):
    """{(collective, element size, call count): plan} for every generated count and the count one pair step above."""
    if (path, n) not in _real:
        specs = []
        for coll in G.BOUNDARY_COLLS[path]:
            for es in SIZES:
                step = G.pair_step(path, coll, es)
                for c, _ in G.boundary_call_counts(path, coll, n, es):
                    specs += [(coll, es, c), (coll, es, c + step)]
        specs = list(dict.fromkeys(specs))
        _real[(path, n)] = dict(zip(specs, plan_many(exe, path, n, specs)))
    return _real[(path, n)]


def check_invariants(path, coll, n, es, c, p):
    """test_planning.py::test_plan_invariants at one count, for whichever kernel the plan names."""
    epp = 16 // es
    g = G.boundary_geom(path, n)
    algo = p["algo"]
    w = (path, coll, n, es, c, p)
    assert 1 <= p["nch"] <= g.cap, w
    if algo in ("ll", "ll128"):
        units = -(-c * es // (8 if algo == "ll" else 56))
        assert (p["nch"] - 1) * p["part"] < units <= p["nch"] * p["part"], w     # no LL channel without a line
        assert p["part"] * (16 if algo == "ll" else 64) <= g.ll_bytes, w
        return
    if "cbdlo" in p and (p["cbdlo"] or p["cbdhi"]):                             # the reference's partition
        assert sum(G._ref_parts(p)) == c and p["nch"] == p["refnch"] * p["sub"], w
        assert p["slice"] % epp == 0 and 0 < p["slice"] <= p["chunk"], w
        return
    whole = algo in ("oneshot", "chain") or p.get("symcoll") == 1
    span = c if whole else p["chunk"]
    assert p["part"] % epp == 0 and p["part"] * p["nch"] >= span, w             # the channels cover a whole block
    if algo != "sym":
        assert p["slice"] % epp == 0 and 0 < p["slice"] <= p["part"], w
        assert p["steps"] == -(-p["part"] // p["slice"]), w
    if coll == "allreduce" and not whole:
        assert p["chunk"] * n >= c and p["chunk"] % epp == 0, w
    if coll == "reduce" and algo == "direct":
        assert p["chunk"] * (n - 1 if n >= 3 else n) >= c and p["chunk"] % epp == 0, w
    if coll in ("reducescatter", "allgather"):
        assert p["chunk"] == c, w


def check_path(path, coll, es, c, p, claimed):
    """The forced path is the planned one; a count built to leave an LL path lands where the default algorithm puts
    it."""
    w = (path, coll, es, c, p, sorted(claimed))
    if path == "RING":
        want = {"allreduce": ("ring", 0), "reducescatter": ("ring", 1), "allgather": ("ring", 2), "reduce": ("chain", 4)}
        assert (p["algo"], p["kind"]) == want[coll], w
    elif path in ("LL", "LL128") and claimed & {"LL capacity: beyond", "LL block not a multiple of 8"}:
        assert p["algo"] == LL_FALLBACK[coll], w
    else:
        assert p["algo"] in PATH_ALGO[path], w
    if path == "TREE":
        assert p["kind"] == 3, w
    if path == "WINDOW_ONESHOT":
        assert p["symcoll"] == 1, w
    if path == "WINDOW":
        assert p["symcoll"] == {"allreduce": 0, "reducescatter": 2, "allgather": 3}[coll], w


@pytest.mark.parametrize("path", list(G.BOUNDARY_ENVS))
def test_generator_hits_what_it_claims(exe, built, path):
    rows = []
    for n in NS:
        real = real_plans(exe, path, n)
        for coll in G.BOUNDARY_COLLS[path]:
            for es in SIZES:
                cmax = G.call_count_cap(coll, n, es)
                gen = G.boundary_call_counts(path, coll, n, es)
                assert gen and len({c for c, _ in gen}) == len(gen)
                plan_of = lambda c: real.get((coll, es, c))
                hit: dict = {}
                for c, claimed in gen:
                    assert 1 <= c <= cmax, (path, coll, n, es, c)
                    p = real[(coll, es, c)]
                    model = G.model_plan(path, coll, n, es, c)
                    assert {k: p[k] for k in PLAN_KEYS if k in p and k in model} == \
                        {k: model[k] for k in PLAN_KEYS if k in p and k in model}, (path, coll, n, es, c, p, model)
                    really = G.classify(path, coll, n, es, c, plan_of)
                    assert claimed <= really, (path, coll, n, es, c, sorted(claimed - really), p)
                    check_invariants(path, coll, n, es, c, p)
                    check_path(path, coll, es, c, p, really)
                    for k in claimed:
                        hit.setdefault(k, []).append(c)
                missing = G.reachable_classes(path, coll, n, es) - set(hit)
                assert not missing, (path, coll, n, es, sorted(missing))
                rows += [(coll, n, es, k, cs) for k, cs in sorted(hit.items())]
    print(f"\n[boundary counts {path}] environment {G.BOUNDARY_ENVS[path]}")
    print(f"{'collective':14} n es {'class':44} call counts")
    for coll, n, es, k, cs in rows:
        print(f"{coll:14} {n} {es:2} {k:44} {cs}")


def test_counts_follow_each_collectives_rule():
    """boundary_counts speaks gpu_cases' convention: a ReduceScatter count is the whole sendbuff, a multiple of n; every
    count carries at most PAYLOAD_CAP bytes per rank; the classes travel with the counts."""
    for path in G.BOUNDARY_ENVS:
        for coll in G.BOUNDARY_COLLS[path]:
            for n in NS:
                for es in SIZES:
                    dtype = G._DTYPE_OF_SIZE[es]
                    got = G.boundary_counts(path, coll, n, dtype)
                    assert [ks for _, ks in got] == [ks for _, ks in G.boundary_call_counts(path, coll, n, es)]
                    for count, _ in got:
                        assert coll != "reducescatter" or count % n == 0
                        assert max(count, G.out_count(coll, n, count)) * es <= G.PAYLOAD_CAP, (path, coll, n, es, count)


def test_many_form_prints_what_the_single_form_prints(exe):
    """plan_test's `many` form against test_planning.py's plan() helper, one process per count, on a few counts of
    every path."""
    for path in G.BOUNDARY_ENVS:
        coll = G.BOUNDARY_COLLS[path][-1]
        counts = [c for c, _ in G.boundary_call_counts(path, coll, 3, 2)][::5]
        many = plan_many(exe, path, 3, [(coll, 2, c) for c in counts])
        for c, m in zip(counts, many):
            assert plan(exe, 3, G._PLAN_FUNC[coll], G._DTYPE_OF_SIZE[2], c, **path_env(path)) == m, (path, coll, c)


# ------------------------------------------------------------------------------------------ the arena comparison

def mock_run(n=3):
    """A numpy mock of a run through the arenas: a few cases of every collective, the images before the run and, as
    `after`, what a correct library leaves: the oracle's results in the output regions and nothing else touched."""
    cases = [G.ArenaCase("allreduce", 2, 0, 37), G.ArenaCase("reducescatter", 6, 0, 3 * 11),
             G.ArenaCase("allgather", 2, 0, 13), G.ArenaCase("reduce", 8, 2, 9, root=1),
             G.ArenaCase("allreduce", 6, 0, 21, inplace=True), G.ArenaCase("allgather", 1, 0, 7, mis=1),
             G.ArenaCase("reducescatter", 2, 0, 3 * 5, inplace=True)]
    sizes = G.arena_layout(cases, n)
    inputs = [G.make_inputs(n, cs.dtype, cs.count, seed=50 + k) for k, cs in enumerate(cases)]
    wants = []
    for cs, ins in zip(cases, inputs):
        exp = G.expected(cs.coll, ins, cs.dtype, cs.op, cs.root)
        wants.append([exp[0] if r == cs.root else None for r in range(n)] if cs.coll == "reduce" else list(exp))
    before = G.arena_images(cases, n, sizes, inputs, wants)
    after = [(s.copy(), r.copy()) for s, r in before]
    for k, cs in enumerate(cases):
        for r in range(n):
            reg = cs.out_region(n, r)
            if reg is not None:
                after[r][1][reg[0]: reg[0] + reg[1]] = np.ascontiguousarray(wants[k][r]).view(np.uint8)
    return cases, before, after, wants


def reported(errs, rank, cs):
    """Every error names the planted fault's rank and count, and there is at least one."""
    assert errs, f"nothing reported for rank {rank} {cs.what()}"
    for e in errs:
        assert e.startswith(f"rank {rank} ") and f" {cs.coll} " in e and f"count={cs.count} " in e, (errs, cs.what())


def test_arena_layout_and_a_correct_mock(built):
    n = 3
    cases, before, after, wants = mock_run(n)
    for cs in cases:
        for off in (cs.send_off, cs.recv_off):
            assert off is None or (off - cs.mis * cs.es) % 16 == 0
    spans = sorted((cs.recv_off, cs.recv_off + cs.recv_bytes(n)) for cs in cases)
    assert spans[0][0] >= G.ARENA_GAP and all(b[0] - a[1] >= G.ARENA_GAP for a, b in zip(spans, spans[1:]))
    assert before[0][1].size - spans[-1][1] >= G.ARENA_GAP
    # the prefill is the complement of the result: an untouched output differs in every byte of every element
    assert G.arena_errors(cases, n, before, before, wants), "an output that was never written must be reported"
    assert G.arena_errors(cases, n, before, after, wants) == []


def test_arena_reports_planted_faults(built):
    n = 3
    cases, before, good, wants = mock_run(n)
    fresh = lambda: [(s.copy(), r.copy()) for s, r in good]
    ar, rs, ag, red, ar_in, ag_mis, rs_in = cases

    # one element written past the end of a slot
    after = fresh()
    off, nb = ar.out_region(n, 1)
    after[1][1][off + nb: off + nb + ar.es] = 0x11
    errs = G.arena_errors(cases, n, before, after, wants)
    reported(errs, 1, ar)
    assert "after the recv slot" in errs[0]

    # the last element left unwritten
    after = fresh()
    off, nb = rs.out_region(n, 2)
    after[2][1][off + nb - rs.es: off + nb] = before[2][1][off + nb - rs.es: off + nb]
    errs = G.arena_errors(cases, n, before, after, wants)
    reported(errs, 2, rs)
    assert "(1 never written)" in errs[0] and f"first at [{rs.count // n - 1}]" in errs[0]

    # the first byte before a slot touched (the slot off 16-byte alignment too)
    for cs, rank in ((ag, 0), (ag_mis, 2)):
        after = fresh()
        after[rank][1][cs.recv_off - 1] ^= 0xFF
        errs = G.arena_errors(cases, n, before, after, wants)
        reported(errs, rank, cs)
        assert "fill byte 1 before the recv slot" in errs[0]

    # two rank blocks of an AllGather exchanged
    after = fresh()
    off, nb = ag.out_region(n, 1)
    blk = ag.count * ag.es
    out = after[1][1][off: off + nb].copy()
    after[1][1][off: off + blk], after[1][1][off + blk: off + 2 * blk] = out[blk: 2 * blk], out[:blk]
    reported(G.arena_errors(cases, n, before, after, wants), 1, ag)

    # a sendbuff byte flipped: out of place (send arena), in place on a Reduce's non-root, in a ReduceScatter's input
    after = fresh()
    after[0][0][red.send_off + 5] ^= 0x01
    errs = G.arena_errors(cases, n, before, after, wants)
    reported(errs, 0, red)
    assert "sendbuff byte 5 changed" in errs[0]
    after = fresh()
    after[0][1][rs_in.recv_off + 1 * (rs_in.count // n) * rs_in.es] ^= 0x80     # rank 0's input block of rank 1
    errs = G.arena_errors(cases, n, before, after, wants)
    reported(errs, 0, rs_in)
    assert "sendbuff byte" in errs[0]
    # a Reduce's recvbuff on a rank that is not the root is never written
    after = fresh()
    after[2][1][red.recv_off] ^= 0x01
    reported(G.arena_errors(cases, n, before, after, wants), 2, red)

    # a ReduceScatter output placed one element late
    after = fresh()
    off, nb = rs.out_region(n, 0)
    after[0][1][off: off + rs.es] = before[0][1][off: off + rs.es]
    after[0][1][off + rs.es: off + nb + rs.es] = good[0][1][off: off + nb]
    errs = G.arena_errors(cases, n, before, after, wants)
    reported(errs, 0, rs)
    assert any("output elements differ" in e for e in errs) and any("after the recv slot" in e for e in errs)


# ------------------------------------------------------------------------------------------ hand-written anchors

# (path, collective, n, element size, call count): fields of the real plan, classes that must hold, classes that must
# not. Worked out by hand from enqueue.cc, not from classify:
#   DIRECT int32 n = 2, slots of 1024 elements, a channel per 128 elements of a block up to 3:
#     12288 = 2 blocks of 6144 = 3 parts of 2048 = 2 slots each; 18432 = 2 x 9216 = 3 parts of 3 slots each;
#     6165: blocks of 3084, the last holds 3081 = 2 parts of 1028 + 1025, one element past a slot;
#     24577: blocks of 12292, parts of 4100 = 5 steps; 4: one block of 4, the second empty; 5: the second holds 1
#   DIRECT int32 n = 3 Reduce (two blocks, none for the root): 4 elements = one full block
#   LL uint8 n = 2, 4 payloads per channel up to 4: 104 bytes = 13 payloads = 4 + 4 + 4 + 1; 65536 bytes = 4 x 2048
#     lines, the capacity; REF_ORDER uint8: 98305 = 6 cells of 16 KiB + 1 element for the last part
ANCHORS = [
    ("DIRECT", "allreduce", 2, 4, 12288, dict(nch=3, part=2048, slice=1024, steps=2, chunk=6144),
     {"part x nch = block", "steps=NSLOTS"}, {"last slice full", "last slice 1", "not a pack multiple"}),
    ("DIRECT", "allreduce", 2, 4, 18432, dict(nch=3, part=3072, slice=1024, steps=3, chunk=9216),
     {"part x nch = block", "steps=NSLOTS+1", "last slice full"}, {"last slice 1"}),
    ("DIRECT", "allreduce", 2, 4, 6165, dict(nch=3, part=1028, slice=1024, steps=2, chunk=3084),
     {"last slice 1", "steps=NSLOTS", "pack+1", "not a pack multiple"}, {"part x nch = block", "last slice full"}),
    ("DIRECT", "allreduce", 2, 4, 24577, dict(nch=3, part=4100, steps=5), {"steps=2NSLOTS+1", "pack+1"}, set()),
    ("DIRECT", "allreduce", 2, 4, 1, dict(nch=1, part=4, steps=1, chunk=4),
     {"count=1", "count<n", "last block empty", "steps=1"}, {"part x nch = block", "last slice full"}),
    ("DIRECT", "allreduce", 2, 4, 4, dict(nch=1, chunk=4), {"last block empty, the others full", "last block empty"},
     {"not a pack multiple", "part x nch = block"}),
    ("DIRECT", "allreduce", 2, 4, 5, dict(nch=1, chunk=4), {"last block 1", "pack+1"}, {"last block empty"}),
    ("DIRECT", "allreduce", 2, 4, 256, dict(nch=1), {"nch 1->2"}, set()),
    ("DIRECT", "reduce", 3, 4, 4, dict(nch=1, chunk=4), {"last block empty, the others full"}, {"last block 1"}),
    ("LL", "allreduce", 2, 1, 104, dict(algo="ll", nch=4, part=4), {"last LL channel one line", "LL bytes mod 8 = 0"},
     {"LL capacity: last inside"}),
    ("LL", "allreduce", 2, 1, 65536, dict(algo="ll", nch=4, part=2048), {"LL capacity: last inside"}, set()),
    ("LL", "allreduce", 2, 1, 65537, dict(algo="oneshot"), {"LL capacity: beyond"}, {"LL bytes mod 8 = 1"}),
    ("LL", "reducescatter", 3, 2, 3, dict(algo="direct"), {"LL block not a multiple of 8"}, {"LL capacity: beyond"}),
    ("REF_ORDER", "allreduce", 2, 1, 98305, dict(algo="direct", cbdhi=1), {"ref cbdHi 1"}, {"ref cbdHi empty"}),
    ("REF_ORDER", "allreduce", 3, 1, 2, dict(algo="direct", cbdlo=2, cbdhi=0),
     {"ref rem=n-1", "ref cbdHi empty", "ref last-loop chunk below a pack"}, {"ref rem=0", "ref rem=1"}),
]


def test_classes_at_hand_computed_counts(exe):
    """classify against expectations worked out by hand (ANCHORS): the predicates the generator and the coverage check
    share are pinned at known counts, the degenerate forms (one channel, one step) excluded."""
    for path, coll, n, es, c, fields, must, must_not in ANCHORS:
        step = G.pair_step(path, coll, es)
        p, nxt = plan_many(exe, path, n, [(coll, es, c), (coll, es, c + step)])
        assert {k: p[k] for k in fields} == fields, (path, coll, n, es, c, p)
        got = G.classify(path, coll, n, es, c, {c: p, c + step: nxt}.get)
        assert must <= got and not (must_not & got), (path, coll, n, es, c, sorted(got))


def test_group_case_is_one_wrapping_batch(exe):
    """The eight counts tests/test_gpu_boundaries.py issues in one group plan as ONE staged launch on the direct
    geometry at n = 2 (plan_test batch): eight ops on a grid of the three channels, their channel ranges chained
    modulo the cap, so that ops start on every channel and several run past the cap and wrap."""
    from tests.test_gpu_boundaries import group_counts
    from tests.test_planning import batch
    counts = group_counts()
    assert len(set(counts)) == 8
    classes = dict(G.boundary_counts("DIRECT", "allreduce", 2, 2))
    assert sum(any(k.startswith("nch ") for k in classes.get(c, ())) for c in counts) == 2
    assert any("steps=NSLOTS+1" in classes.get(c, ()) for c in counts)
    launches = batch(exe, 2, *[f"ar:2:{c}" for c in counts], **path_env("DIRECT"))
    assert len(launches) == 1, launches
    l, = launches
    assert (l["algo"], l["ops"], l["grid"]) == ("direct", 8, 3), l
    nchs = [G.model_plan("DIRECT", "allreduce", 2, 4, c)["nch"] for c in counts]
    off = 0
    for (o, k), nch in zip(l["ranges"], nchs):
        assert (o, k) == (off, nch), (l, nchs)
        off = (off + nch) % 3
    assert {o for o, _ in l["ranges"]} == {0, 1, 2} and sum(o + k > 3 for o, k in l["ranges"]) >= 2, l
