"""GPU tests of the numerics of the device API's reduce-copy fold (include/nccl_device_reduce_copy.h):
sources fold in index order; __half and __hip_bfloat16 accumulate in fp32 under nccl::utility::OpSum with one
round-to-nearest-even at the end; everything else, every user RedOp included, folds in T; nSrc == 1 copies bits.

Inputs are gpu_cases.edge_inputs (every fp16 / bf16 pattern, fp32 / fp64 at the edges of every exponent, against 18
partners: ties from both sides, overflow, cancellation, subnormals, signed zeros, every NaN, +-Inf) and sets cut from
them that tell a wrong fold from the right one (edge_sets): rounding twice instead of once, a fold out of source order,
the group-of-four boundaries of the source loop. tests/test_device_rc_cpu.py::test_edge_sets_discriminate checks on the
CPU that the sets do tell these apart, and that the NaN cap holds for every one of them.

The reference (ref_sum, ref_fold_T) is numpy on storage bits, with no torch conversion: up (fp16: astype(float32);
bf16: bits << 16), float32 addition, down (fp16: astype(float16); bf16: the header's integer formula). Comparison is the
project's rule: gpu_cases.same_bits (every bit; a NaN where the reference has one) under the 10 % NaN cap, plus bit for
bit the elements with exactly one NaN among the sources and none made by the fold (the result is that input's bits).
The user max and the nSrc == 1 copy compare every element bit for bit. Every test prints the share of elements it
compared bit for bit."""
import time

import numpy as np
import pytest

from tests.test_gpu_broadcast import FILL, _destroy, _torch
from tests.test_gpu_device_api import _cs, _setup, _teardown
from tests.test_gpu_device_rc import GUARD, TYPES, _kernels, inplace_case, lsa_case

pytestmark = pytest.mark.gpu

KINDS = {"half": 6, "bfloat16": 9, "float": 7, "double": 8}      # name -> gpu_cases' type code
SHORT = ("half", "bfloat16")
MANY_NSRC = (4, 5, 6, 9, 16)      # around the source loop's groups of four: 1 + 3, 1 + 4, 1 + 4 + 1, 1 + 8, 1 + 15
NAN_CAP = 0.10


def _G():
    from tests import gpu_cases as G
    return G


# ---------------------------------------------------------------- the reference fold, on storage arrays

def up(kind, x):
    """Storage (uint16 bits of half / bfloat16, float32, float64) -> the accumulate type's values."""
    if kind == "half":
        return x.view(np.float16).astype(np.float32)
    if kind == "bfloat16":
        return (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return x


def down(kind, f):
    """The accumulate type's values -> storage: nearest even; a bf16 NaN keeps its top bits and is made quiet."""
    if kind == "half":
        with np.errstate(over="ignore"):
            return f.astype(np.float16).view(np.uint16)
    if kind == "bfloat16":
        u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
        nan = (u & 0x7fffffff) > 0x7f800000
        rounded = (u + 0x7fff + ((u >> 16) & 1)) >> 16
        return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)
    return f


def _one_nan(kind, srcs, made):
    """Elements with exactly one NaN among the sources and no NaN made by the fold (Inf - Inf): compared bit for bit."""
    return (np.stack([np.isnan(up(kind, s)) for s in srcs]).sum(0) == 1) & ~made


def ref_sum(kind, srcs, upto=None):
    """{k: (the header's sum of srcs[0..k), the elements of it with one defined NaN)} for every k in `upto` (default:
    only len(srcs)). half / bfloat16: folded in float32, rounded once; float / double: a + b in T. k == 1: the bits."""
    upto = set(upto or [len(srcs)])
    out = {}
    if 1 in upto:
        out[1] = (srcs[0].copy(), np.isnan(up(kind, srcs[0])))
    with np.errstate(over="ignore", invalid="ignore"):
        acc = up(kind, srcs[0])
        made = np.zeros(acc.size, dtype=bool)
        for i in range(1, len(srcs)):
            s = up(kind, srcs[i])
            new = acc + s
            assert new.dtype == acc.dtype
            made |= np.isnan(new) & ~np.isnan(acc) & ~np.isnan(s)
            acc = new
            if i + 1 in upto:
                out[i + 1] = (down(kind, acc), _one_nan(kind, srcs[:i + 1], made))
    return out


def ref_fold_T(kind, srcs, op):
    """(a user RedOp's fold of srcs in T — convert up, apply, convert down at every step — and its one-NaN elements).
    op: "sum" (a + b) or "max" (a < b ? b : a, a select of the operands' bits)."""
    acc = srcs[0].copy()
    made = np.zeros(acc.size, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in srcs[1:]:
            a, b = up(kind, acc), up(kind, s)
            if op == "max":
                acc = np.where(a < b, s, acc)
            else:
                new = a + b
                made |= np.isnan(new) & ~np.isnan(a) & ~np.isnan(b)
                acc = down(kind, new)
    return acc, _one_nan(kind, srcs, made)


def nan_share(kind, want):
    return float(np.isnan(up(kind, want)).mean())


def differing_share(kind, x, y):
    """The share of the elements that are a NaN in neither x nor y on which the two differ in any bit."""
    G = _G()
    ok = ~(np.isnan(up(kind, x)) | np.isnan(up(kind, y)))
    return float((G._raw(x)[ok] != G._raw(y)[ok]).mean())


# ---------------------------------------------------------------- the input sets

_sets: dict = {}


def edge_sets(kind):
    """{name: (sources, the nSrc to run them at)}, storage arrays, read-only and shared. ln is the base list's length,
    r0 and E are ranks 0 and 1 of edge_inputs (E: 18 blocks of ln partners), a is block 0 of r0:
      edge    edge_inputs(3) at nSrc 2 and 3 (its first two sources are edge_inputs(2))
      dr      [a, h, h], h = half an ulp of a (E's block 6): a + h is a tie that rounds to even and the second h is lost
              where the fold rounds per step; in fp32 a + 2h is the next value.            (half, bfloat16)
      dr1     [a, h | 1, h]: just above the tie (block 7)                                    (half, bfloat16)
      order   [a, swapped, -a] (blocks 9 and 3): [a, -a, swapped] gives `swapped` exactly    (half, bfloat16)
      many    r0, then E rotated left by 0 .. 14 blocks: 16 sources, run at MANY_NSRC
      many17  (half, bfloat16) `many` and r0 again: more sources than pointers kept in registers"""
    if kind in _sets:
        return _sets[kind]
    G = _G()
    dt = KINDS[kind]
    r0, E, r2 = G.edge_inputs(dt, 3)
    two = G.edge_inputs(dt, 2)
    assert np.array_equal(G._raw(two[0]), G._raw(r0)) and np.array_equal(G._raw(two[1]), G._raw(E))
    ln = G._edge_base(dt).size
    assert r0.size == G.EDGE_BLOCKS * ln == {"half": 1179648, "bfloat16": 1179648, "float": 147456,
                                             "double": 589824}[kind]
    sets = {"edge": ([r0, E, r2], (2, 3))}
    if kind in SHORT:
        block = lambda b: E[(b - 1) * ln: b * ln]
        a, h, h1, nega, swapped = r0[:ln], block(6), block(6) | np.uint16(1), block(3), block(9)
        assert np.array_equal(h1, block(7)) and np.array_equal(nega, a ^ np.uint16(0x8000))
        sets["dr"] = ([a, h, h], (3,))
        sets["dr1"] = ([a, h1, h], (3,))
        sets["order"] = ([a, swapped, nega], (3,))
    many = [r0] + [np.roll(E, -i * ln) for i in range(15)]
    sets["many"] = (many, MANY_NSRC)
    if kind in SHORT:
        sets["many17"] = (many + [r0], (17,))
    for srcs, _ in sets.values():
        for s in srcs:
            s.setflags(write=False)
    _sets[kind] = sets
    return sets


def copy_set(kind):
    """The base list's raw patterns, signalling NaNs left in."""
    G = _G()
    dt = KINDS[kind]
    return G._edge_base(dt).view(G.oracle.NP_STORAGE[dt])


# ---------------------------------------------------------------- the device side

class Arena:
    """Up to `nsrc` sources and 2 destinations of `total` elements each, in two device buffers allocated once: source
    i at element i * displ of the source buffer, destination d at i * displ plus a shift of the destination buffer,
    guard bytes in front, between and behind."""

    def __init__(self, kind, total, nsrc):
        torch = _torch()
        self.kind, self.total = kind, total
        self.code, self.elt = TYPES[kind]
        self.dt = KINDS[kind]
        self.displ = (total * self.elt + 32 + 15) // 16 * 16 // self.elt
        self.src = torch.full((GUARD + nsrc * self.displ * self.elt + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.fill = torch.full((GUARD + 2 * self.displ * self.elt + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.dst = self.fill.clone()
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0
        self.sbase = self.src.data_ptr() + GUARD
        self.stab = torch.tensor([self.sbase + i * self.displ * self.elt for i in range(nsrc)], dtype=torch.int64,
                                 device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.host = None
        self.compared = self.exact = 0

    def placements(self):
        """Destination shifts in bytes: 16-byte aligned like the sources; 4 bytes off (the 4-byte packs of the 2-byte
        types, the scalar loop for float); one element off (the scalar loop)."""
        return sorted({0, self.elt} | ({4} if self.elt <= 4 else set()))

    def load(self, srcs):
        torch = _torch()
        assert all(s.size <= self.total for s in srcs)
        raw = np.full(self.src.numel(), FILL, dtype=np.uint8)
        for i, s in enumerate(srcs):
            at = GUARD + i * self.displ * self.elt
            raw[at:at + s.nbytes] = s.view(np.uint8)
        self.src.copy_(torch.from_numpy(raw))
        self.host = raw

    def sources_intact(self):
        return bool(np.array_equal(self.src.cpu().numpy(), self.host))

    def dtab(self, dshift):
        torch = _torch()
        base = self.dst.data_ptr() + GUARD + dshift
        return base, torch.tensor([base, base + self.displ * self.elt], dtype=torch.int64, device="cuda")

    def results(self, dshift, ndst, count, like):
        """The destinations' elements after a launch, whether every other byte kept its fill; the buffer is refilled."""
        torch = _torch()
        torch.cuda.synchronize()
        raw = self.dst.cpu().numpy()
        used = np.zeros(raw.size, dtype=bool)
        got = []
        for d in range(ndst):
            at = GUARD + dshift + d * self.displ * self.elt
            used[at:at + count * self.elt] = True
            got.append(raw[at:at + count * self.elt].copy().view(like.dtype))
        clean = bool(np.all(raw[~used] == FILL))
        self.dst.copy_(self.fill)
        return got, clean

    def local(self, coop, form, nsrc, ndst, count, dshift, want, one, what):
        """One rc_local launch against (want, one); returns errors."""
        dbase, dtab = self.dtab(dshift)
        rc = _kernels().rc_local(self.code, coop, 1, form, self.stab.data_ptr(), dtab.data_ptr(), self.sbase,
                                 self.displ, dbase, self.displ, nsrc, ndst, count, self.stream)
        assert rc == 0, f"launch failed: {rc}"
        got, clean = self.results(dshift, ndst, count, want)
        errs = []
        for d, g in enumerate(got):
            errs += self.compare(g, want[:count], one[:count], f"{what} destination {d}")
        if not clean:
            errs.append(f"{what}: bytes around the destinations were written")
        return errs

    def compare(self, got, want, one, what):
        """The project's rule; `one` None: every element bit for bit."""
        G = _G()
        self.compared += want.size
        if one is None:
            self.exact += want.size
            bad = np.nonzero(G._raw(got) != G._raw(want))[0]
            if bad.size:
                return [f"{what}: {bad.size} of {want.size} elements differ, first at {bad[:5].tolist()} got "
                        f"{[hex(int(v)) for v in G._raw(got)[bad[:3]]]} want "
                        f"{[hex(int(v)) for v in G._raw(want)[bad[:3]]]}"]
            return []
        self.exact += int((~np.isnan(up(self.kind, want)) | one).sum())
        return G.edge_errors(got, want, one, self.dt, what)

    def report(self, name, t0):
        print(f"\n[{name} {self.kind}] {self.exact} of {self.compared} result elements compared bit for bit "
              f"({100.0 * self.exact / max(self.compared, 1):.2f} %), {time.time() - t0:.1f} s")


def _capped(kind, want, what):
    assert nan_share(kind, want) <= NAN_CAP, f"{what}: more than 10 % of the reference's result is NaN"
    assert _G().nan_cap_ok(want, KINDS[kind])


LOCAL_FORMS = ((0, 1), (1, 1), (4, 2))      # (rc_local's form, nDst): ReduceSum lambda, strided; ReduceSumCopy strided


# ---------------------------------------------------------------- 1. the sum through the local forms

@pytest.mark.parametrize("kind", list(KINDS))
def test_local_sum_edge(built, kind):
    """Every set through ncclLocalReduceSum (lambda, strided) and ncclLocalReduceSumCopy (nDst = 2): the CTA of 256
    threads at the three placements; the warp and the 72-thread CTA on edge3 aligned; the thread coop on the first
    2 * ln elements of edge3."""
    t0 = time.time()
    sets = edge_sets(kind)
    total = sets["edge"][0][0].size
    ar = Arena(kind, total, 16)
    errs = []
    for name in ("edge", "dr", "dr1", "order", "many"):
        if name not in sets:
            continue
        srcs, nsrcs = sets[name]
        ar.load(srcs)
        count = srcs[0].size
        ref = ref_sum(kind, srcs, nsrcs)
        for nsrc in nsrcs:
            want, one = ref[nsrc]
            _capped(kind, want, f"{kind} {name} nSrc={nsrc}")
            for dshift in ar.placements():
                for form, ndst in LOCAL_FORMS:
                    errs += ar.local(2, form, nsrc, ndst, count, dshift, want, one,
                                     f"{kind} {name} nSrc={nsrc} form={form} shift={dshift}")
            if name == "edge" and nsrc == 3:
                ln = count // _G().EDGE_BLOCKS
                for coop, cnt in ((1, count), (3, count), (0, 2 * ln)):
                    for form, ndst in LOCAL_FORMS:
                        errs += ar.local(coop, form, nsrc, ndst, cnt, 0, want, one,
                                         f"{kind} {name} nSrc={nsrc} form={form} coop={coop}")
        if not ar.sources_intact():
            errs.append(f"{kind} {name}: a source was written")
        if len(errs) > 20:
            break
    ar.report("local sum", t0)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("kind", SHORT)
def test_more_than_16_sources_edge(built, kind):
    """17 sources (`many` and r0 again) through ncclLocalReduceSum's lambda form: the element-at-a-time loop, same
    fold, same rounding."""
    t0 = time.time()
    srcs, (n,) = edge_sets(kind)["many17"]
    count = srcs[0].size
    ar = Arena(kind, count, n)
    ar.load(srcs)
    want, one = ref_sum(kind, srcs)[n]
    _capped(kind, want, f"{kind} many17")
    errs = []
    for dshift in (0, ar.elt):
        errs += ar.local(2, 0, n, 1, count, dshift, want, one, f"{kind} many17 shift={dshift}")
    if not ar.sources_intact():
        errs.append(f"{kind} many17: a source was written")
    ar.report("17 sources", t0)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 2. the copy

@pytest.mark.parametrize("kind", list(KINDS))
def test_copy_preserves_every_pattern(built, kind):
    """ncclLocalCopy (lambda and strided, nDst = 2) and ncclLocalReduceSum with nSrc = 1 (lambda and strided) move every
    pattern of the base list unchanged, signalling NaNs included, at the three placements."""
    t0 = time.time()
    x = copy_set(kind)
    G = _G()
    bits = G._raw(x)
    emax, mant = {"half": (0x7c00, 0x3ff), "bfloat16": (0x7f80, 0x7f), "float": (0x7f800000, 0x7fffff),
                  "double": (0x7ff << 52, (1 << 52) - 1)}[kind]
    quiet = (mant + 1) >> 1
    snan = ((bits & emax) == emax) & ((bits & mant) != 0) & ((bits & quiet) == 0)
    assert snan.any(), "the copy set has no signalling NaN"
    ar = Arena(kind, x.size, 1)
    ar.load([x])
    errs = []
    for dshift in ar.placements():
        for form, ndst in ((2, 2), (3, 2), (0, 1), (1, 1)):
            dbase, dtab = ar.dtab(dshift)
            rc = _kernels().rc_local(ar.code, 2, 1, form, ar.stab.data_ptr(), dtab.data_ptr(), ar.sbase, ar.displ,
                                     dbase, ar.displ, 1, ndst, x.size, ar.stream)
            assert rc == 0, f"launch failed: {rc}"
            got, clean = ar.results(dshift, ndst, x.size, x)
            what = f"{kind} copy form={form} shift={dshift}"
            for d, g in enumerate(got):
                errs += ar.compare(g, x, None, f"{what} destination {d}")
            if not clean:
                errs.append(f"{what}: bytes around the destinations were written")
    if not ar.sources_intact():
        errs.append(f"{kind} copy: the source was written")
    ar.report("copy", t0)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 3. user RedOps fold in T

@pytest.mark.parametrize("kind", list(KINDS))
def test_user_ops_fold_in_T(built, kind):
    """ncclLsaReduceLsaCopy with a user a + b (not nccl::utility::OpSum) and a user max on edge3, dr, dr1 and order: the
    sum is the per-step fold in T — on dr it differs from the fp32-accumulate result on at least 40 % of the elements —
    and max is a < b ? b : a on every element, NaNs and +-0 included."""
    t0 = time.time()
    k = _kernels()
    sets = edge_sets(kind)
    ar = Arena(kind, sets["edge"][0][0].size, 3)
    errs = []
    for name in ("edge", "dr", "dr1", "order"):
        if name not in sets:
            continue
        srcs, _ = sets[name]
        ar.load(srcs)
        count = srcs[0].size
        _, dtab = ar.dtab(0)
        for op, fn in (("sum", k.rc_usersum), ("max", k.rc_max)):
            want, one = ref_fold_T(kind, srcs, op)
            if op == "sum":
                _capped(kind, want, f"{kind} {name} user sum")
            rc = fn(ar.code, ar.stab.data_ptr(), 3, dtab.data_ptr(), 2, count, ar.stream)
            assert rc == 0, f"launch failed: {rc}"
            got, clean = ar.results(0, 2, count, want)
            what = f"{kind} {name} user {op}"
            for d, g in enumerate(got):
                errs += ar.compare(g, want, one if op == "sum" else None, f"{what} destination {d}")
            if not clean:
                errs.append(f"{what}: bytes around the destinations were written")
            if op == "sum" and name == "dr":
                share = differing_share(kind, got[0], ref_sum(kind, srcs)[3][0])
                print(f"\n[user ops {kind}] dr: the user sum differs from the fp32-accumulate sum on "
                      f"{100 * share:.1f} % of the non-NaN elements")
                if share < 0.40:
                    errs.append(f"{what}: differs from the fp32-accumulate result on only {100 * share:.1f} %")
        if not ar.sources_intact():
            errs.append(f"{kind} {name}: a source was written")
    ar.report("user ops", t0)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 4. across ranks

@pytest.mark.parametrize("kind", SHORT)
def test_lsa_edge_in_process(built, kind):
    """edge3 across 3 ranks of one process: ncclLsaReduceSum (lambda), ncclLsaReduceSumCopy and
    ncclLsaReduceSumLsaCopy at grid 4, and the in-place ncclLsaReduceSumCopy: the cross-rank wiring folds in rank order
    with the same rounding."""
    t0 = time.time()
    n = 3
    xs, _ = edge_sets(kind)["edge"]
    count = xs[0].size
    want, one = ref_sum(kind, xs)[n]
    _capped(kind, want, f"{kind} edge3")
    G = _G()
    seen = [0, 0]

    def fold(k, srcs):
        assert k == kind and srcs is xs
        return want

    def check(got, w, what):
        seen[0] += w.size
        seen[1] += int((~np.isnan(up(kind, w)) | one).sum())
        return G.edge_errors(got, w, one, KINDS[kind], what)

    cs = _cs(n)
    rs = _setup(cs, count * TYPES[kind][1], 4)
    errs = lsa_case(rs, n, kind, count, (0, 10, 15), (4,), 0, inputs=xs, fold=fold, check=check)
    if not errs:
        errs += inplace_case(rs, n, kind, count, 4, 0, forms=(10,), inputs=xs, fold=fold, check=check)
    _teardown(rs, destroy_comms=False)
    _destroy(cs)
    print(f"\n[lsa edge {kind}] {seen[1]} of {seen[0]} result elements compared bit for bit "
          f"({100.0 * seen[1] / max(seen[0], 1):.2f} %), {time.time() - t0:.1f} s")
    assert not errs, "\n".join(errs[:20])
