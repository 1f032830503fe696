"""The precondition of tests/test_gpu_line_stage.py, checked without a GPU: on the oracle's
evaluation counts of its ray set, a host model of the march's line stages (nrt_kernels.h
LineStage: the slot table of kStageSlots lines, first free slot, evict slot 0, complete-line
flush, drain) under one wave's job hand-out evicts slots and reopens evicted lines -- and still
writes every ray's word exactly once.  Nothing here comes from the kernel."""
import pytest
import torch

from tests.report import report
from tests.test_gpu_line_stage import (FAR, INSIDE, MARGIN, SIZES, SLOW, SLOW_MIN_STEPS,
                                       eviction_rays)

STAGE_SLOTS = 8  # kStageSlots


class StageModel:
    """LineStage's bookkeeping: tag / msk per slot, and how often each ray's word is written."""

    def __init__(self, limit):
        self.tag = [-1] * STAGE_SLOTS
        self.msk = [0] * STAGE_SLOTS
        self.limit = limit
        self.written = {}
        self.evictions = self.full_lines = self.reopened = 0
        self.evicted = set()

    def flush(self, q):
        for off in range(16):
            if (self.msk[q] >> off) & 1:
                ray = self.tag[q] * 16 + off
                self.written[ray] = self.written.get(ray, 0) + 1
        self.tag[q], self.msk[q] = -1, 0

    def put(self, ray):
        line, off = ray >> 4, ray & 15
        if line in self.tag:
            q = self.tag.index(line)
        else:
            if -1 in self.tag:
                q = self.tag.index(-1)
            else:
                q = 0
                self.evictions += 1
                self.evicted.add(self.tag[0])
                self.flush(0)
            self.reopened += line in self.evicted
            self.tag[q], self.msk[q] = line, 0
        self.msk[q] |= 1 << off
        n = self.limit - line * 16
        if self.msk[q] == (0xffff if n >= 16 else (1 << n) - 1):
            self.full_lines += 1
            self.flush(q)

    def drain(self):
        for q in range(STAGE_SLOTS):
            if self.tag[q] >= 0:
                self.flush(q)


def run_wave(steps, lines, P, lanes=16):
    """One wave of the launch-queue march over the chunks `lines` (16 jobs each, job k = ray k):
    every pass retires the lanes whose march is over (their words go to the stage, in lane
    order), hands the waiting lanes the next jobs in lane order, and evaluates once."""
    jobs = [r for ln in lines for r in range(ln * 16, min(ln * 16 + 16, P))]
    stage = StageModel(P)
    ray, left, nxt = [-1] * lanes, [0] * lanes, 0
    while True:
        for l in range(lanes):
            if ray[l] >= 0 and left[l] == 0:
                stage.put(ray[l])
                ray[l] = -1
        for l in range(lanes):
            if ray[l] < 0 and nxt < len(jobs):
                ray[l], left[l] = jobs[nxt], steps[jobs[nxt]]
                nxt += 1
        if all(r < 0 for r in ray):
            break
        for l in range(lanes):
            if ray[l] >= 0:
                left[l] -= 1
    stage.drain()
    return stage, jobs


@pytest.mark.parametrize("hidden", [128, 256])
def test_eviction_rays_are_what_the_gpu_test_needs(hidden):
    rs = eviction_rays(hidden)
    kind, steps, hit, t, margin = (rs[k] for k in ("kind", "steps", "hit", "t", "margin"))
    assert bool((kind[::16] == SLOW).all())
    slow, ins, far = kind == SLOW, kind == INSIDE, kind == FAR
    assert int(ins.sum()) + int(far.sum()) + int(slow.sum()) == kind.numel()
    report(f"eviction_rays[{hidden}]", slow_steps_min=steps[slow].min(), slow_steps_max=steps[slow].max(),
           slow_margin_min=margin[slow].min(), slow_hits=int(hit[slow].sum()),
           far_steps_min=steps[far].min(), far_steps_max=steps[far].max(),
           margin_min=margin.min())
    assert steps[slow].min().item() >= SLOW_MIN_STEPS
    assert margin[slow].min().item() >= MARGIN
    # inside origins: a hit at the first evaluation, t == 0; far origins: a miss
    assert bool((steps[ins] == 1).all()) and bool(hit[ins].all()) and bool((t[ins] == 0).all())
    assert not hit[far].any() and bool((t[far] >= 10.0).all())
    assert margin[~slow].min().item() >= MARGIN  # (no other ray's decision is close either)


@pytest.mark.parametrize("lanes", [16, 32])  # the FP32 / split engines' tile, the FP16 engine's
@pytest.mark.parametrize("P,blocks", SIZES)
@pytest.mark.parametrize("hidden", [128, 256])
def test_host_model_evicts_and_reopens(hidden, P, blocks, lanes):
    steps = eviction_rays(hidden)["steps"][:P].tolist()
    nlines = (P + 15) // 16
    for name, lines in (("consecutive", range(nlines)), ("every 8th", range(0, nlines, 8))):
        stage, jobs = run_wave(steps, list(lines), P, lanes)
        report(f"line_stage_host[{hidden},{P},{lanes},{name}]", evictions=stage.evictions,
               reopened=stage.reopened, full_lines=stage.full_lines)
        assert stage.evictions >= 1 and stage.reopened >= 1, name
        assert sorted(stage.written) == jobs and set(stage.written.values()) == {1}, name
