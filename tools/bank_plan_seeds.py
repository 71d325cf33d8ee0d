"""Choose the seeds of tests/bank_plan.py's tables: a greedy search over candidate seeds for the ones whose plans, together, meet the coverage
conditions that tests/test_bank_plan_cases.py asserts.  Prints SEEDS_Q15 / SEEDS_F32 to paste into tests/bank_plan.py; the host state machine
alone, no oracle and no GPU.    python tools/bank_plan_seeds.py [candidates]
The committed seeds are the output of the default, bank_plan.CANDIDATES candidates; the greedy choice is deterministic."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import bank_plan as P  # noqa: E402


def items(d, f32):
    """the coverage a plan brings, as a multiset of items: (what, key) -> how many"""
    it = {}
    for k, n in d["kinds"].items():
        it[("kind", k)] = n
    for k, n in d["refusal_kinds"].items():
        it[("refusal", k)] = n
    for p in d["pairs"]:
        it[("pair", p)] = 1
    for o in d["orders"]:
        it[("order", o)] = 1
    for g in d["gated_on"]:
        it[("on", g)] = 1
    for g in d["gated_off"]:
        it[("off", g)] = 1
    for k in P.WANTED_COUNTS:
        if not (f32 and k in ("reset_mid_cadence", "lms_decimated", "agc_stepping")):          # (asserted over the Q15 table)
            it[("count", k)] = d[k]
    return it


def need():
    """what tests/test_bank_plan_cases.py asserts, from the same constants"""
    w = {("kind", k): 4 for k in P.KINDS + ("call_iq",)}
    w.update({("refusal", k): n for k, n in P.WANTED_REFUSALS.items()})
    w.update({("pair", p): 1 for p in P.wanted_pairs()})
    w.update({("order", o): 1 for o in P.wanted_orders()})
    w.update({("on", g): 1 for g in P.WANTED_GATED_ON})
    w.update({("off", g): 1 for g in P.WANTED_GATED_OFF})
    w.update({("count", k): n for k, n in P.WANTED_COUNTS.items()})
    return w


def usable(d):
    return d["refusals"] >= 1 and d["short"] >= 2 and d["calls"] >= 6 and 10 <= d["steps"] <= 14 and d["max_gen"] < 16


def choose(n, f32, left, cands):
    pool = {}
    for s in cands:
        d = P.survey(P.draw(s, f32))
        if usable(d):
            pool[s] = items(d, f32)
    chosen = []
    for _ in range(n):
        best = max(pool, key=lambda s: (sum(min(v, left.get(k, 0)) for k, v in pool[s].items()), -s))
        chosen.append(best)
        for k, v in pool.pop(best).items():
            if k in left:
                left[k] = max(0, left[k] - v)
    return sorted(chosen)


if __name__ == "__main__":
    ncand = int(sys.argv[1]) if len(sys.argv) > 1 else P.CANDIDATES
    left = need()
    # the fp32 plans first (what they cover of the common conditions the Q15 plans need not): five with the two cascade sections (even seeds), five without
    f32 = sorted(choose(5, True, left, range(0, ncand, 2)) + choose(5, True, left, range(1, ncand, 2)))
    q15 = choose(32, False, left, range(ncand))
    print("SEEDS_Q15 = %r" % (tuple(q15),))
    print("SEEDS_F32 = %r" % (tuple(f32),))
    print("unmet:", {k: v for k, v in left.items() if v})
