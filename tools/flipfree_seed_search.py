"""Seed search for tests/test_gpu_flipfree_gradients.py (CPU only): for every shape of tests/_flipfree_reference.py and
for G and GC, the first seed suffix s0, s1, ... whose fp64 reference train step is flip-free (margin rule and conditions:
docstring of tests/_flipfree_reference.py) and leaves at most 5 % of the gradient tensors with a norm below 1e-6.

    python tools/flipfree_seed_search.py [--shapes b1w8,b2w8] [--limit 4000] [--jobs 8]     search, print the table
    python tools/flipfree_seed_search.py --check      re-derive the margins of the committed table (SEEDS in the test module)
    ... --write    also rewrite the reference half of profiles/flipfree_gradients.txt

A candidate is first run forward only (fp64 and fp32, ~0.2 s); one that passes the margin rule there gets the full check
with gradients and the eval forward.  Candidates are tried in order and the first that passes wins, whatever --jobs is."""
import argparse
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import _flipfree_reference as R  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "flipfree_gradients.txt")
MARK = "# ---- measured on the GPU"


def tiny_share(shape, concat, suffix):
    g = R.oracle_train(shape, concat, suffix, torch.float64)["grads"]
    return sum(1 for t in g if t.norm().item() < 1e-6) / len(g)


def passes(shape, concat, suffix):
    return not R.flip_free_violations(shape, concat, suffix) and tiny_share(shape, concat, suffix) <= 0.05


def _screen(job):
    shape, concat, n = job
    torch.set_num_threads(1)
    t64, t32 = (R.traced_forward(shape, concat, f"s{n}", d) for d in (torch.float64, torch.float32))
    a, k = R.achieved_margin(R.margins(t64, t32))
    return n, a >= R.M and k >= R.M


def search(shape, concat, limit, jobs):
    """(suffix, candidates tried) of the first passing seed, or (None, limit)"""
    with mp.Pool(jobs) as pool:
        for n, ok in pool.imap(_screen, ((shape, concat, n) for n in range(limit)), chunksize=4):
            if ok and passes(shape, concat, f"s{n}"):
                pool.terminate()
                return f"s{n}", n + 1
            R.oracle_train.cache_clear(); R.oracle_eval.cache_clear()
    return None, limit


def row(sid, concat, suffix):
    shape = R.SHAPES[sid]
    m = R.margins(*(R.oracle_train(shape, concat, suffix, d) for d in (torch.float64, torch.float32)))
    a, k = R.achieved_margin(m)
    lo = min(v / rms for v, _, rms, _ in m["act"])
    err = max(e / rms for _, e, rms, _ in m["act"])
    gap = min(g for g, _ in m["argmax"])
    return (f"{sid:6s} {'gc' if concat else 'g':3s} {suffix:7s} inputs {sum(n for *_, n in m['act']):7d}   "
            f"min|u64|/rms {lo:.2e}   max fp32 err/rms {err:.2e}   activation margin {a:8.1f}   "
            f"top-two gap {gap:.2e}   arg-max margin {k:10.1f}   tiny-norm share {tiny_share(shape, concat, suffix):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(R.SHAPES))
    ap.add_argument("--limit", type=int, default=4000)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    rows = []
    if a.check:
        from test_gpu_flipfree_gradients import SEEDS
        for (sid, variant), suffix in SEEDS.items():
            bad = R.flip_free_violations(R.SHAPES[sid], variant == "gc", suffix)
            rows.append(row(sid, variant == "gc", suffix) + ("" if not bad else "   NOT FLIP-FREE: " + "; ".join(bad)))
            print(rows[-1], flush=True)
    else:
        for sid in a.shapes.split(","):
            for concat in (False, True):
                suffix, tried = search(R.SHAPES[sid], concat, a.limit, a.jobs)
                if suffix is None:
                    rows.append(f"{sid:6s} {'gc' if concat else 'g':3s} no flip-free seed among s0 .. s{a.limit - 1} at M = {R.M:g}")
                else:
                    rows.append(row(sid, concat, suffix) + f"   (candidate {tried})")
                print(rows[-1], flush=True)
    if a.write:
        tail = ""
        if os.path.exists(PROFILE):
            old = open(PROFILE).read()
            tail = old[old.index(MARK):] if MARK in old else ""
        with open(PROFILE, "w") as f:
            f.write(f"# flip-free references (tools/flipfree_seed_search.py, CPU only): M = {R.M:g}; margins = min over the sites of\n"
                    "# min|u64| / max|u32-u64| (activations) and top-two gap / (2 max|p32-p64|) (arg-max)\n")
            f.write("\n".join(rows) + "\n" + tail)


if __name__ == "__main__":
    main()
