"""What the wrappers of inference.py do around the network per frame, pinned against a record.

One recorder (tests/_recorder.py) that forwards every call to the real library stands in as `_L` of ops.py, frame_ops.py,
highres.py and the modules of the later stages (guided.py, sgm.py, ground.py, stixel.py, temporal.py).  Every case of
tests/_inference_cases.py `wrapper_cases()` is one instance, eager (graph=False, so every launch of every frame comes through
the recorder; SGMInference has no model and no graph) in the 32 x 64 frame, fed three frames: a full frame, an image smaller
than the frame, the full frame again (small, full, full for KittiInferenceTemporal) -- no first-use allocation falls into the
last call.  A frame is a pair, or a pair and the case's third item (a hint map, a pose).  tests/golden/inference_trace.json
holds per case, for that LAST call:

    frame   the (entry point, arguments) sequence of the calls that came through every module but ops.py: the glue
    ops     of the calls through ops.py (the network), the launch count per entry point and a SHA-256 of the sequence
    allocs  the growth of torch.cuda.memory_stats()["allocation.all.allocated"] across the call, less the part that falls
            inside the two 2D networks (feature extraction, guidance)
    returns per returned array its dtype and shape (None for a missing one)

Why the 2D networks are taken out of the allocation count: they are PyTorch convolutions, served by MIOpen, and whether a
convolution allocates a workspace follows the solver MIOpen picks on the machine at hand: they are the one part of a frame
whose allocations the project does not make itself.  Seen with one and the same code on several MI355X machines: a pass of
the network made 316 allocations inside the 2D networks on some and 385 on others, in every case alike, and 224 outside
them on all.

    python tests/test_gpu_inference_trace.py --record COMMIT              rewrites the file, noting COMMIT as its origin
    python tests/test_gpu_inference_trace.py --record-missing COMMIT      records only the cases the file does not have yet and
                                                                          notes COMMIT for each under "added_on"; every other
                                                                          byte of the file stays

The file is a record of behaviour: a reordered or added launch, a changed argument or one more allocation per frame shows here.
The cases of the seven older classes (plain, confidence, lr, filtered, highres, 3d, color) were recorded on the commit before
those wrappers were restructured (the file's "recorded_on").  The cases of KittiInferenceGuided, KittiInferenceGround,
KittiInferenceStixels, KittiInferenceTemporal and SGMInference were recorded on the commit before the frame pipeline was taken
apart from the network (the file's "added_on"), with that commit's inference.py.  Re-record only in a change that means to alter
what a frame does, and read the diff."""
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


def _run(case, rec, marks, miopen):
    from dcanet_amd import inference
    cls, ctor, call = case.cls, case.ctor, case.call
    if case.model:
        infer = getattr(inference, cls)(C.model(), graph=False, **C.FRAME, **ctor)
    else:
        infer = getattr(inference, cls)(**ctor)
    frames = C.pairs(np.random.default_rng(7), case.sizes)
    if case.items is not None:
        frames = [pair + (item,) for pair, item in zip(frames, case.items(np.random.default_rng(8), case.sizes))]
    for frame in frames[:2]:
        infer(*frame, **call)
    torch.cuda.synchronize()
    del rec.calls[:], marks[:], miopen[:]
    before = _allocated()
    res = infer(*frames[2], **call)
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


def _trace_all(setattr_, only=None):
    """{case id: its trace} of every case (only: of the cases named)"""
    from dcanet_amd import _lib, frame_ops, ground, guided, highres, ops, sgm, stixel, temporal
    rec, marks = Recorder(_lib.load()), []

    def glue():                  # every module but ops.py calls `_L().entry(...)`: the next recorded call is the glue's
        marks.append(len(rec.calls))
        return rec

    setattr_(ops, "_L", lambda: rec)
    for module in (frame_ops, highres, guided, sgm, ground, stixel, temporal):
        setattr_(module, "_L", glue)
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
    return {case.id: _run(case, rec, marks, miopen) for case in C.wrapper_cases() if only is None or case.id in only}


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


def _dump(obj):
    return json.dumps(obj, sort_keys=True, separators=(",", ":"))


def _report(traces):
    print(len(traces), "cases,", sum(len(t["frame"]) for t in traces.values()), "glue calls,",
          sum(sum(t["ops"]["launches"].values()) for t in traces.values()), "launches,", os.path.getsize(GOLDEN_FILE), "bytes")


def record(commit):
    traces = _trace_all(setattr)
    with open(GOLDEN_FILE, "w") as f:
        f.write(_dump({"recorded_on": commit, "cases": traces}) + "\n")
    _report(traces)


def record_missing(commit):
    """adds the cases the file lacks, each with `commit` under "added_on"; the entries the file has stay byte for byte"""
    with open(GOLDEN_FILE) as f:
        text = f.read()
    golden = json.loads(text)
    assert text == _dump(golden) + "\n", "the file is not in the form `record` writes"
    missing = [c.id for c in C.wrapper_cases() if c.id not in golden["cases"]]
    traces = _trace_all(setattr, missing)
    golden["cases"].update(traces)
    golden.setdefault("added_on", {}).update({cid: commit for cid in traces})
    with open(GOLDEN_FILE, "w") as f:
        f.write(_dump(golden) + "\n")
    _report(traces)


if __name__ == "__main__":
    for flag, fn in (("--record", record), ("--record-missing", record_missing)):
        if flag in sys.argv:
            fn(sys.argv[sys.argv.index(flag) + 1])
