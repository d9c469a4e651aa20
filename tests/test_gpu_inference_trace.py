"""What the wrappers of inference.py do around the network per frame, pinned against a record.

One recorder (tests/_recorder.py) that forwards every call to the real library stands in as `_L` of ops.py, frame_ops.py and
highres.py.  Every case of tests/_inference_cases.py `wrapper_cases()` is one instance, eager (graph=False, so every launch of
every frame comes through the recorder) in the 32 x 64 frame, fed three pairs: a full frame, an image smaller than the frame,
the full frame again -- no first-use allocation falls into the last call.  tests/golden/inference_trace.json holds per case,
for that LAST call:

    frame   the (entry point, arguments) sequence of the calls that came through frame_ops.py and highres.py: the glue
    ops     of the calls through ops.py (the network), the launch count per entry point and a SHA-256 of the sequence
    allocs  the growth of torch.cuda.memory_stats()["allocation.all.allocated"] across the call, less the part that falls
            inside the two 2D networks (feature extraction, guidance)
    returns per returned array its dtype and shape (None for a missing one)

Why the 2D networks are taken out of the allocation count: they are PyTorch convolutions, served by MIOpen, and whether a
convolution allocates a workspace follows the solver MIOpen picks on the machine at hand: they are the one part of a frame
whose allocations the project does not make itself.  Seen with one and the same code on several MI355X machines: a pass of
the network made 316 allocations inside the 2D networks on some and 385 on others, in every case alike, and 224 outside
them on all.

    python tests/test_gpu_inference_trace.py --record COMMIT      rewrites the file, noting COMMIT as its origin

The file was recorded on the commit before the wrappers were restructured (see its "recorded_on") and is a record of behaviour:
a reordered or added launch, a changed argument or one more allocation per frame shows here.  Re-record it only in a change that
means to alter what a frame does, and read the diff."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _inference_cases as C  # noqa: E402
from _recorder import Recorder  # noqa: E402

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "inference_trace.json")


def _allocated():
    return torch.cuda.memory_stats()["allocation.all.allocated"]


def _run(cls, ctor, call, sizes, rec, marks, miopen):
    from dcanet_amd import inference
    infer = getattr(inference, cls)(C.model(), graph=False, **C.FRAME, **ctor)
    pairs = C.pairs(np.random.default_rng(7), sizes)
    for left, right in pairs[:2]:
        infer(left, right, **call)
    torch.cuda.synchronize()
    del rec.calls[:], marks[:], miopen[:]
    before = _allocated()
    res = infer(*pairs[2], **call)
    allocs = _allocated() - before - sum(miopen)
    torch.cuda.synchronize()
    print(f"{cls} {ctor} {call}: {allocs} allocations, and {sum(miopen)} inside the 2D networks")
    glue = set(marks)
    ops_calls = [c for i, c in enumerate(rec.calls) if i not in glue]
    names = [c[0] for c in ops_calls]
    return {"frame": [rec.calls[i] for i in marks],
            "ops": {"launches": {n: names.count(n) for n in sorted(set(names))},
                    "sha256": hashlib.sha256(json.dumps(ops_calls).encode()).hexdigest()},
            "allocs": allocs,
            "returns": [None if a is None else [str(a.dtype), list(a.shape)] for a in (res if isinstance(res, tuple) else (res,))]}


def _trace_all(setattr_):
    from dcanet_amd import _lib, frame_ops, highres, ops
    rec, marks = Recorder(_lib.load()), []

    def glue():                  # frame_ops.py and highres.py call `_L().entry(...)`: the next recorded call is theirs
        marks.append(len(rec.calls))
        return rec

    setattr_(ops, "_L", lambda: rec)
    setattr_(frame_ops, "_L", glue)
    setattr_(highres, "_L", glue)
    setattr_(torch.backends.cudnn, "deterministic", True)      # MIOpen convolutions of the 2D networks
    miopen = []                  # allocations made inside the two 2D networks, per call of one
    for module in (C.model().feature_extraction, C.model().guidance):
        def forward(*args, _real=module.forward):
            before = _allocated()
            try:
                return _real(*args)
            finally:
                miopen.append(_allocated() - before)
        setattr_(module, "forward", forward)
    return {cid: _run(cls, ctor, call, sizes, rec, marks, miopen) for cid, cls, ctor, call, sizes in C.wrapper_cases()}


@pytest.mark.gpu
def test_inference_trace(monkeypatch):
    with open(GOLDEN_FILE) as f:
        golden = json.load(f)["cases"]
    got = json.loads(json.dumps(_trace_all(monkeypatch.setattr)))
    assert sorted(got) == sorted(golden)
    bad = []
    for cid in got:
        for key in got[cid]:
            if got[cid][key] != golden[cid][key]:
                bad.append(f"{cid}, {key}:\n    recorded {golden[cid][key]}\n    now      {got[cid][key]}")
    assert not bad, f"{len(bad)} records changed:\n" + "\n".join(bad)


def record(commit):
    traces = _trace_all(setattr)
    with open(GOLDEN_FILE, "w") as f:
        json.dump({"recorded_on": commit, "cases": traces}, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(len(traces), "cases,", sum(len(t["frame"]) for t in traces.values()), "glue calls,",
          sum(sum(t["ops"]["launches"].values()) for t in traces.values()), "launches,", os.path.getsize(GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record(sys.argv[sys.argv.index("--record") + 1])
