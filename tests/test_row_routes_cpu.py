"""
Which kernel family a row transform of the C ABI runs (csrc/swiftly_rowroute.h, ``choose_row_route``), without a GPU:
``tests/native/row_route_dump.cpp`` includes only that header and prints what it answers; this test compiles it with the
compiler of the library's host code.

Expectations: ``tests/golden/row_routes.txt`` holds calls and the answers RECORDED from the ladder this header replaced
(``run_rows`` / ``run_rows_chunk`` / ``try_col_pass`` / ``try_row_pass`` of csrc/swiftly_abi.hip, ``launch_one`` of
csrc/fft_rows_impl.h and ``make_plan`` of csrc/swiftly_abi_coltransform.hip before it, run on the CPU with launchers that
print their name and mode instead of launching; profiles/README.md) -- one line per distinct (facts that mattered, answer)
that a grid of 13.3 million recorded calls met.  A line is ``<the 46 RowCall fields> -> kind mode single_store_window
refusal``, in the order of the dump program; the mode of a route other than ``Lean`` is ``-``: the recording shows no mode
where no launcher takes one.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd", "csrc")

CALL = ("dbl n logn sub all_j rowfast in_rs1 out_rs1 nrows in_cs out_cs tab_use nbatch rm in_rowmap st_rowmap row_win ld_win ld_win2 "
        "st_win st_win2 st_win_bs ld_a ld_len ld_c ld_mod st_a st_len st_c st_mod accumulate real_in real_out raw_ld raw_st tw tw_m1 "
        "tw_m2 tw_h1 tw_h2 mixed blu col_gs col_c128 col_f64 col_f64_stages").split()
ROUTE = "kind mode single_store_window refusal".split()
KINDS = ["ColPass", "Lean", "Band32kPlain", "Split32k", "Band32kMapped", "Band64k", "LongRowsF64", "Generic", "FourStep", "Mixed",
         "Bluestein", "Empty", "Refused"]
REFUSALS = ["", "Length", "Stride", "NoConvolution", "NoTable", "RealInDecomposed", "RealOutNoStore", "64kLeanOnly",
            "LongMappedLoadOnly", "NoGenericInstance"]
#: what exists in complex64 only (the lean kernels, the 65536-point refusal) and in complex128 only (the long-row pair)
FLOAT_ONLY_KINDS = {"ColPass", "Lean", "Band32kPlain", "Split32k", "Band32kMapped", "Band64k"}
DOUBLE_ONLY_KINDS = {"LongRowsF64"}
FLOAT_ONLY_REFUSALS = {"64kLeanOnly"}
DOUBLE_ONLY_REFUSALS = {"LongMappedLoadOnly"}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the compiled program as a function: list of request lines -> list of answer lines"""
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    exe = str(tmp_path_factory.mktemp("row_routes") / "row_route_dump")
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "row_route_dump.cpp"), "-o", exe], check=True, timeout=300)

    def run(requests):
        res = subprocess.run([exe], input="\n".join(requests) + "\n", stdout=subprocess.PIPE, text=True, check=True, timeout=120)
        return res.stdout.splitlines()

    return run


@pytest.fixture(scope="module")
def golden():
    """[(call dict, answer dict)]; a ``-`` of the file is None"""
    rows = []
    with open(os.path.join(ROOT, "tests", "golden", "row_routes.txt"), encoding="utf-8") as fh:
        for line in fh:
            call, answer = (side.split() for side in line.split("->"))
            assert len(call) == len(CALL) and len(answer) == len(ROUTE), line
            rows.append((dict(zip(CALL, map(int, call))), {k: None if v == "-" else int(v) for k, v in zip(ROUTE, answer)}))
    assert 500 < len(rows) < 3000
    return rows


def choose(dump, calls):
    answers = dump(["route " + " ".join(str(c[k]) for k in CALL) for c in calls])
    assert len(answers) == len(calls)
    return [dict(zip(ROUTE, map(int, line.split()))) for line in answers]


def call(n, **facts):
    """a RowCall with everyday values: 8 rows along the contiguous axis, one item, identity maps, every table there"""
    logn = n.bit_length() - 1 if n & (n - 1) == 0 else -1
    c = dict.fromkeys(CALL, 0)
    c.update(n=n, logn=logn, nrows=8, in_cs=1, out_cs=1, nbatch=1, ld_len=n, ld_mod=n, st_len=n, st_mod=n, tw=1, tw_m1=1, tw_m2=1,
             tw_h1=1, tw_h2=1)
    c.update(facts)
    assert set(c) == set(CALL)
    return c


def real_instances(dump):
    """{(dbl, logn): (real load, real store)} of the generic kernel"""
    keys = [(dbl, logn) for dbl in (0, 1) for logn in range(0, 21)]
    return dict(zip(keys, (tuple(map(int, line.split())) for line in dump([f"real {d} {l}" for d, l in keys]))))


def test_golden_answers(dump, golden):
    got = choose(dump, [c for c, _ in golden])
    for (c, want), have in zip(golden, got):
        assert {k: have[k] for k, v in want.items() if v is not None} == {k: v for k, v in want.items() if v is not None}, c
        assert (want["mode"] is not None) == (KINDS[want["kind"]] == "Lean")
        assert (want["refusal"] != 0) == (KINDS[want["kind"]] == "Refused")
    # what the file has to hold: every route kind and every refusal, in both precisions where it exists
    for dbl in (0, 1):
        kinds = {KINDS[w["kind"]] for c, w in golden if c["dbl"] == dbl}
        assert kinds == set(KINDS) - (DOUBLE_ONLY_KINDS, FLOAT_ONLY_KINDS)[dbl]
        refusals = {REFUSALS[w["refusal"]] for c, w in golden if c["dbl"] == dbl and w["refusal"]}
        assert refusals == set(REFUSALS[1:]) - (DOUBLE_ONLY_REFUSALS, FLOAT_ONLY_REFUSALS)[dbl]
    assert {w["mode"] for c, w in golden if KINDS[w["kind"]] == "Lean"} == {0, 1, 2}
    assert {(KINDS[w["kind"]], w["single_store_window"]) for c, w in golden if w["single_store_window"] or KINDS[w["kind"]] == "Band64k"} == \
           {("Band32kMapped", 1), ("Band64k", 0), ("Band64k", 1)}
    # every refusal is there on its own: a line that meets that refusal's condition and no other's
    inst = real_instances(dump)
    lim = 1 << 32
    conditions = {
        "Length": lambda c: c["logn"] >= 0 and not 3 <= c["logn"] <= (15 if c["dbl"] else 16),
        "Stride": lambda c: c["n"] * c["in_cs"] >= lim or c["n"] * c["out_cs"] >= lim,
        "NoConvolution": lambda c: c["logn"] < 0 and not c["mixed"] and not c["blu"],
        "NoTable": lambda c: c["logn"] >= 0 and not c["tw"],
        "RealInDecomposed": lambda c: c["real_in"] and (c["sub"] or c["rowfast"] or c["raw_ld"]),
        "RealOutNoStore": lambda c: c["real_out"] and (c["sub"] or c["rowfast"] or c["st_rowmap"] or c["accumulate"] or
                                                       (not c["dbl"] and c["logn"] >= 13)),
        "64kLeanOnly": lambda c: not c["dbl"] and c["logn"] == 16,
        "LongMappedLoadOnly": lambda c: c["dbl"] and not c["rowfast"] and c["logn"] > 13 and (c["sub"] or c["raw_ld"]),
        "NoGenericInstance": lambda c: (c["real_in"] and not inst[c["dbl"], c["logn"]][0]) or (c["real_out"] and not inst[c["dbl"], c["logn"]][1]),
    }
    for dbl in (0, 1):
        for name, cond in conditions.items():
            if name in (DOUBLE_ONLY_REFUSALS, FLOAT_ONLY_REFUSALS)[dbl]:
                continue
            assert any(c["dbl"] == dbl and REFUSALS[w["refusal"]] == name and cond(c) and
                       not any(other(c) for k, other in conditions.items() if k != name) for c, w in golden), (dbl, name)
    # and the conditions of a refusal hold on every line refused with it
    for c, w in golden:
        if w["refusal"]:
            assert conditions[REFUSALS[w["refusal"]]](c), (c, w)


def test_invariants_of_the_route(dump, golden):
    for c, w in golden:
        kind = KINDS[w["kind"]]
        if c["real_in"] or c["real_out"]:
            assert kind not in ("ColPass", "FourStep", "Mixed", "Bluestein"), c
        if kind == "LongRowsF64":
            assert c["dbl"] and not c["rowfast"] and c["logn"] in (14, 15)
        if kind == "Band64k":
            assert c["logn"] == 16 and not c["dbl"]
        if kind == "FourStep":
            assert c["rowfast"] and c["logn"] >= 9
        if kind in FLOAT_ONLY_KINDS:
            assert not c["dbl"] and not c["sub"]
        if kind in ("Mixed", "Bluestein", "Refused") and w["refusal"] in (0, 3):
            assert (c["logn"] < 0) == (kind != "Refused" or REFUSALS[w["refusal"]] == "NoConvolution")
        if kind == "Empty":
            assert c["nrows"] <= 0 or c["nbatch"] <= 0
    # real rows where no entry point sends them -- along the strided axis, at a length that is not a power of two: refused,
    # where the ladder before this header would have run the column passes, the radix-Q pass or Bluestein on them as if
    # they were complex (the one difference to the recording, which holds no such call)
    assert not [c for c, _ in golden if (c["real_in"] or c["real_out"]) and (c["rowfast"] or c["logn"] < 0)]
    odd = [call(n, dbl=dbl, rowfast=rowfast, in_rs1=rowfast, out_rs1=rowfast, in_cs=8 if rowfast else 1, out_cs=8 if rowfast else 1, mixed=mixed,
                blu=1, **{real: 1})
           for real in ("real_in", "real_out") for dbl in (0, 1) for n, rowfast, mixed in ((256, 1, 0), (2048, 1, 0), (768, 0, 1), (1000, 0, 0))]
    for c, have in zip(odd, choose(dump, odd)):
        assert KINDS[have["kind"]] == "Refused" and REFUSALS[have["refusal"]] == ("RealInDecomposed" if c["real_in"] else "RealOutNoStore"), c


def test_real_instances_and_lengths_exist_once(dump):
    inst = real_instances(dump)
    for logn in range(0, 21):
        assert inst[0, logn] == (6 <= logn <= 12, 6 <= logn <= 12)  # complex64: 64 .. 4096 points (8192 and more: the lean kernels)
        assert inst[1, logn] == (6 <= logn <= 13, 6 <= logn <= 13)  # complex128: 64 .. 8192 points
    lengths = dump([f"length {d} {l} {m} {b}" for d in (0, 1) for l in range(-1, 21) for m in (0, 1) for b in (0, 1)])
    want = [int((3 <= l <= (15 if d else 16)) if l >= 0 else bool(m or b)) for d in (0, 1) for l in range(-1, 21) for m in (0, 1) for b in (0, 1)]
    assert list(map(int, lengths)) == want
    # the launcher of the generic kernel asks the same predicates; it and the other kernel headers state no range of their own
    with open(os.path.join(CSRC, "fft_rows_impl.h"), encoding="utf-8") as fh:
        text = fh.read()
    assert "if constexpr (generic_has_real_load(sizeof(R) == 8, LOGN))" in text
    assert "if constexpr (generic_has_real_store(sizeof(R) == 8, LOGN))" in text
    assert not re.search(r"LOGN\s*[<>]=?\s*(\d|k[A-Z])", text)
    for name in ("kMaxLogNDouble", "kMaxLogNDoubleRows", "kTwoPassMinLog", "kRowPassMinLog", "kRowPassMaxLog", "kLongLogN1", "kColPassMinLog",
                 "kColPassMaxLog", "kColF64MinLog", "kColPassMaxLogF64"):
        found = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))
                 and re.search(r"const(expr)? int " + name + r"\b", open(os.path.join(CSRC, f), encoding="utf-8").read())]
        assert found == ["swiftly_rowroute.h"], (name, found)


def test_column_pass_split(dump):
    """single pass or four-step, the halves, the range and the float64 stages: literal expectations"""
    def split(logn, gs=0, c128=0, f64=0, stages=7, W=8):
        return tuple(map(int, dump([f"split {logn} {gs} {c128} {f64} {stages} {W}"])[0].split()))

    for logn in range(0, 22):
        status, two, l1, l2, f64, one, a, b = split(logn)
        assert (status, two, f64, one, a, b) == (0 if 2 <= logn <= 20 else 1, int(logn > 10), 0, 0, 0, 0)
        assert (l1, l2) == ((logn // 2, logn - logn // 2) if logn > 10 else (logn, 0))
        assert split(logn, gs=1)[1] == int(logn > 9) and split(logn, c128=1)[1] == int(logn > 9)
        # complex128 storage: float64 instances or nothing (32 .. 512 points per pass)
        c128 = split(logn, c128=1)
        ok = (5 <= logn <= 9) or (logn > 9 and 5 <= logn // 2 and logn - logn // 2 <= 9)
        assert c128[0] == (0 if ok else (1 if not 2 <= logn <= 20 else 2)), (logn, c128)
        if ok:
            assert c128[4:] == (1, 1, 1, 1)
    assert split(9, f64=1, stages=4)[4:] == (1, 1, 0, 0) and split(9, gs=1, f64=1)[4] == 0 and split(8, gs=1, f64=1)[4] == 1
    assert split(15, f64=1, stages=3)[4:] == (1, 0, 1, 1) and split(10, f64=1)[4] == 0 and split(20, f64=1)[4] == 0
    assert split(15, W=1 << 17)[0] == 3 and split(15, W=(1 << 17) - 1)[0] == 0 and split(10, W=1 << 30)[0] == 0  # scratch of a four-step < 2^32 elements


def test_capability_rules_promise_a_route(dump):
    """Where ``why_not_real_facets`` / ``_f64`` / ``_out`` / ``_out_f64`` (csrc/swiftly_caps.h, asked through
    ``swiftly_hip_supports``) say yes, the row call behind ``prepare_facet_band_real*`` / ``finish_facet_band_real*`` is not
    refused -- for every log2(yN) 0 .. 20 and a representative facet.  (complex64 at yN 16384 .. 65536: the forward K1 has
    its own ladder above the band kernel and does not ask this chooser.)"""
    from ska_sdp_exec_swiftly_amd import _lib

    lib = _lib.load()
    asked = {}
    for log_yn in range(0, 21):
        yn = 1 << log_yn
        for feature, dtype, forward in ((_lib.FEATURE_REAL_FACETS, _lib.C64, True), (_lib.FEATURE_REAL_FACETS_F64, _lib.C128, True),
                                        (_lib.FEATURE_REAL_FACETS_OUT, _lib.C64, False), (_lib.FEATURE_REAL_FACETS_OUT_F64, _lib.C128, False)):
            # a configuration the rule accepts at this yN, if there is one: m = 128 / 256 with a sum_finish instance, or m = yN
            sizes = [(N, xM) for N, xM in ((2 * yn, 256), (4 * yn, 1024), (yn, yn)) if N % xM == 0 and lib.swiftly_hip_supports(feature, dtype, N, yn, xM, 0)]
            if not sizes:
                continue
            dbl = int(dtype == _lib.C128)
            if forward and not dbl and 14 <= log_yn <= 16:
                continue
            yb = max(2, (yn * 3 // 4) & ~1)
            tables = dict(tw_m1=int(log_yn in (14, 15, 16)), tw_m2=int(log_yn == 15), tw_h1=int(log_yn >= 9), tw_h2=int(log_yn >= 9))
            calls = []
            for a in (0, yn // 2 + 3):  # aligned, rotated
                if forward:
                    for row_win in (0, 1):
                        calls.append(call(yn, dbl=dbl, real_in=1, ld_a=a, ld_len=yb, ld_mod=yb, ld_win=1, row_win=row_win, **tables))
                else:
                    for mask in (0, 1):
                        for band in ((0, yn), ((yn - 5) % yn, yn // 2 + 1)):
                            calls.append(call(yn, dbl=dbl, real_out=1, ld_a=(-band[0]) % yn, ld_len=band[1], ld_mod=band[1], st_a=a, st_len=yb,
                                              st_mod=yb, st_win=mask, st_win2=1, **tables))
            for c, have in zip(calls, choose(dump, calls)):
                assert KINDS[have["kind"]] not in ("Refused", "Empty"), (feature, log_yn, c, have)
                asked.setdefault((feature, dbl), set()).add((log_yn, KINDS[have["kind"]]))
    assert {k: sorted(v) for k, v in asked.items()} == {
        (_lib.FEATURE_REAL_FACETS, 0): [(l, "Generic") for l in range(7, 13)] + [(13, "Lean")],
        (_lib.FEATURE_REAL_FACETS_F64, 1): [(l, "Generic") for l in range(7, 14)] + [(14, "LongRowsF64"), (15, "LongRowsF64")],
        (_lib.FEATURE_REAL_FACETS_OUT, 0): sorted([(l, "Generic") for l in range(6, 13)] + [(13, "Lean"), (14, "Lean"), (15, "Band32kMapped"),
                                                                                          (16, "Band64k")]),
        (_lib.FEATURE_REAL_FACETS_OUT_F64, 1): [(l, "Generic") for l in range(6, 14)] + [(14, "LongRowsF64"), (15, "LongRowsF64")],
    }
