"""The fp32 accuracy gate has teeth: deliberately degraded builds of the library FAIL it.

`make -C minimal-sdr_amd mutants` (part of __graft_entry__.build(); never the product library) compiles msdr_api.hip three more times with
-DMSDR_MUTATE=k:
    1  the lo pieces of the chain's tap fragments zeroed: the xh x Bl product is gone, the taps keep 11 bits  (error ~ 2e-4)
    2  the taps rounded to 16 significant bits before they are split                                          (error ~ 4e-6: INSIDE the
       north-star's 1e-5 -- only the contract's float64 clause, applied to every case, sees it)
    3  time segments start their cascade from zero state: no re-convergence over a warm-up                    (error at segment boundaries)
    4  the row-local threshold of the envelope cascade's scan loosened: 2^-40 read as 2^-16.  Chosen on the CPU together with the census
       case "env_s2_scan1_near_threshold" (tests/test_f32_flavour_cases.py): a 5400 Hz low-pass of Q 1.46 (the product's threshold is
       near Q 0.71) in front of the Q 15 notch.  The criterion's left side there is 4.5e-6 of its right: the product build scans 4 x 4
       (env_scan 1), the mutant takes section 0 out of the scan (env_scan 2).  A float64 model of the row-local kernel on the case's
       own rows puts the mutant 8.4e-6 ... 8.6e-6 from float64: above 3 x the rows' bound (2.4e-6) and below 1e-5 -- the first clause
       passes, only the float64 clause can see it.  (The same model reads 1.70e-5 at Q 1.5478, where the kernel measured 1.69e-5.)
       The mutant changes the flavour as well, which the census's info() assertion would catch without saying anything about
       accuracy: its child runs with MSDR_CENSUS_ACCURACY_ONLY=1 and must fail on the float64 clause and on nothing else.
    5  the lo halves of the cascade's response fragments zeroed (rl, and the lo halves of lf / df): the folded cascade's correction
       keeps 11 bits.  Must fail EVERY census entry that runs a folded cascade, SSB or envelope (picked from the table by its flavour bits).
Each test below runs gate tests in a child process against one mutant (MSDR_LIB) and asserts that the child PASSES -- marked
xfail(strict=True): the expected outcome is a failure of the gate, and a mutant that slips through turns this test red.  Mutants 1-3
are held against the fuzzers' gate AND against the flavour census (tests/test_gpu_f32_flavours.py), 4 and 5 against the census.  The
a-priori error model behind each clause of the contract is DESIGN.md 5."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUT = {1: ["tests/test_gpu_f32_contract.py::test_fp32_contract_on_the_fuzzers_cases"],
       2: ["tests/test_gpu_f32_contract.py::test_fp32_contract_on_the_fuzzers_cases"],
       3: ["tests/test_gpu_chain.py::test_chain_f32_time_segments_vs_sequential"]}
CENSUS = "tests/test_gpu_f32_flavours.py::test_flavour_runs_and_meets_both_clauses[%s]"


def _folded_entries():
    import test_gpu_f32_flavours as census
    from gpuhelp import msdr
    return [e["name"] for e in census.flavours(census.oracle()) if e["flavour"] & (msdr.FLAVOUR_SSB_FOLD | msdr.FLAVOUR_ENV_FOLD)]


# (mutant, census entry): each child must fail
CENSUS_MUT = [(1, "ssb_s0"), (2, "ssb_s0"), (3, "ssb_s2_folded_segmented"), (4, "env_s2_scan1_near_threshold")] + [(5, n) for n in _folded_entries()]


class ChildDidNotRun(Exception):
    """The child process gave no verdict (import error, library not loaded): NOT the assertion failure the xfail marks expect."""


def _verdict(r):
    lines = r.stdout.splitlines()
    if not lines or not ("passed" in r.stdout or "failed" in r.stdout) or "error" in lines[-1]:
        raise ChildDidNotRun(r.stdout[-2000:])
    return r.returncode


def _run(lib, tests, extra_env=None):
    env = dict(os.environ, MSDR_LIB=lib)
    env.pop("MSDR_CENSUS_ACCURACY_ONLY", None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + tests, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)


def test_the_product_library_passes_the_same_gate_in_a_child_process():
    """The control: the very same child invocations with the product library are green (so a red mutant run is the mutant's doing)."""
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
    r = _run(lib, sorted({t for ts in MUT.values() for t in ts}) + sorted({CENSUS % e for _, e in CENSUS_MUT}))
    assert r.returncode == 0, r.stdout[-3000:]
    r = _run(lib, [CENSUS % "env_s2_scan1_near_threshold"], {"MSDR_CENSUS_ACCURACY_ONLY": "1"})
    assert r.returncode == 0 and "FLAVOUR DIFFERS" not in r.stdout, r.stdout[-3000:]


def _mutant(k):
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib_mut%d" % k, "libmsdr.so")
    if not os.path.exists(lib):
        pytest.skip("mutant %d not built (make -C minimal-sdr_amd mutants)" % k)
    return lib


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="a degraded build must NOT pass the accuracy gate")
def test_a_degraded_build_passes_the_gate(k):
    r = _run(_mutant(k), MUT[k])
    print(r.stdout[-1500:])
    assert _verdict(r) == 0             # (a child that did not run the tests raises ChildDidNotRun: an error, not the expected failure)


_CHILD = {}


def _census_child(k, entry):
    if (k, entry) not in _CHILD:
        _CHILD[(k, entry)] = _run(_mutant(k), [CENSUS % entry, "-s"], {"MSDR_CENSUS_ACCURACY_ONLY": "1"} if k == 4 else None)
    return _CHILD[(k, entry)]


@pytest.mark.parametrize("k,entry", CENSUS_MUT)
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="a degraded build must NOT pass the flavour census")
def test_a_degraded_build_passes_the_census(k, entry):
    r = _census_child(k, entry)
    print(r.stdout[-2500:])
    assert _verdict(r) == 0


def test_mutant_4_fails_on_the_float64_clause_alone():
    """Not an expected failure: the child of mutant 4 must have run on the row-local scan (the flavour differs: printed, not asserted) and
    have failed on the census's float64 assertion -- not on the flavour, and not on the 1e-5 clause, which this defect stays inside."""
    r = _census_child(4, "env_s2_scan1_near_threshold")
    assert _verdict(r) != 0 and "FLAVOUR DIFFERS" in r.stdout, r.stdout[-3000:]
    assert "float64 clause" in r.stdout and "'first clause'" not in r.stdout, r.stdout[-3000:]
