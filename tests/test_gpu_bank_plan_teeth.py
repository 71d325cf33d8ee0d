"""Do the bank's plans (tests/test_gpu_bank_plans.py) have teeth in the host state machine?

`make -C minimal-sdr_amd mutants` (part of __graft_entry__.build(); never the product library) compiles msdr_api.hip twice more for this file,
each build changing one VALUE of the host's bookkeeping -- no address, size, lifetime or launch geometry:
  -DMSDR_MUTATE=6   a phase-continuous msdr_chain_set_nco_channels (phase == NULL) rebases the phase at nco_T + 1 instead of nco_T
  -DMSDR_MUTATE=7   msdr_chain_reset leaves the spectrum's cadence counter as it was
As in tests/test_gpu_f32_teeth.py, each mutant runs the plans in a child process (MSDR_LIB) and the test that asserts the child PASSES is
marked xfail(strict=True): a mutant that slips through turns it red.  Beside that, not as expected failures: mutant 6 fails EVERY Q15 plan that
holds a retune without phases and no other, and nothing in tests/test_bank_plan_cases.py (the model never sees the library's bookkeeping);
mutant 7 fails exactly the plans in which a reset moves the cadence where a call can see it (tests/bank_plan.py's survey), and no other."""
import os
import re
import subprocess
import sys

import pytest

import bank_plan as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = "tests/test_gpu_bank_plans.py"
_CHILD = {}


class ChildDidNotRun(Exception):
    """The child process gave no verdict (import error, library not loaded): NOT the assertion failure the xfail marks expect."""


def _lib(k):
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib_mut%d" % k if k else "lib", "libmsdr.so")
    if not os.path.exists(lib):
        pytest.skip("mutant %d not built (make -C minimal-sdr_amd mutants)" % k)
    return lib


def _child(k, marker="gpu", tests=PLANS):
    """(return code, the seeds of the plans that failed, stdout) of the plans under library k (0: the product)"""
    if (k, tests) not in _CHILD:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", marker, "-p", "no:cacheprovider", "-rfE", tests], cwd=ROOT,
                           env=dict(os.environ, MSDR_LIB=_lib(k)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        lines = r.stdout.splitlines()
        if not lines or not ("passed" in r.stdout or "failed" in r.stdout) or "error" in lines[-1]:
            raise ChildDidNotRun(r.stdout[-2000:])
        _CHILD[(k, tests)] = (r.returncode, {int(m) for m in re.findall(r"^FAILED \S+::test_plan\[(\d+)\]", r.stdout, re.M)}, r.stdout)
    return _CHILD[(k, tests)]


def _seeds(key):
    return {p.seed for p in P.plans_q15() if P.survey(p)[key]}


def test_the_product_library_passes_the_plans_in_a_child_process():
    """The control: the very same child invocation with the product library is green (so a red mutant run is the mutant's doing)."""
    rc, failed, out = _child(0)
    assert rc == 0 and not failed, out[-3000:]


@pytest.mark.parametrize("k", [6, 7])
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="a build with a defect in the host state machine must NOT pass the plans")
def test_a_mutated_build_passes_the_plans(k):
    rc, failed, out = _child(k)
    print(out[-1500:])
    assert rc == 0


def test_mutant_6_fails_every_plan_with_a_phase_continuous_retune_and_no_other():
    rc, failed, out = _child(6)
    want = _seeds("phaseless")
    assert len(want) >= 8 and failed == want, (sorted(failed ^ want), out[-3000:])
    rc, _, out = _child(6, "not gpu", "tests/test_bank_plan_cases.py")
    assert rc == 0, out[-3000:]


def test_mutant_7_fails_the_plans_whose_reset_moves_the_cadence_and_no_other():
    rc, failed, out = _child(7)
    want = _seeds("reset_mid_cadence")
    assert len(want) >= 2 and failed == want, (sorted(failed ^ want), out[-3000:])
