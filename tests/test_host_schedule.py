"""Properties of the host-batch schedules (swmi_host_granules_for, the granules score_host_batch issues), no device needed.
One child process per knob setting, since the library reads its environment once: the production score group (2^24 pairs) and
two test groups (SWMI_TEST_SCORE_GROUP, one with a small steady granule through SWMI_HOST_MIN_GRANULE).  For every entry and a
sweep of n around 4 x steady, every multiple of steady inside a tail, and one, two and three score groups, plus ragged sizes:
  - each score group's granules sum to exactly that group, so group boundaries fall on granule boundaries;
  - every granule is at least one pair;
  - each group is scheduled on its own: its granules are the schedule of a batch of that group's size;
  - the largest granule of the whole batch is the largest of the full group's schedule and the tail group's schedule -- the
    two sizes score_host_batch sizes its slot buffers from (the tail's can be the larger one)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG

CHILD = r"""
import json, os, random, sys
sys.path.insert(0, %r)
import swmi
group = int(os.environ.get("SWMI_TEST_SCORE_GROUP", 1 << 24))
steady = int(os.environ.get("SWMI_HOST_MIN_GRANULE", 1 << 17))
sizes = set()
for base in (4 * steady, group, 2 * group, 3 * group):
    for d in (-4097, -4096, -1, 0, 1, 4095, 4096):
        sizes.add(base + d)
for k in range(1, group // steady + 1):                 # every multiple of steady inside a tail, and 4 x steady inside one
    for d in (-1, 0, 1):
        sizes.add(group + k * steady + d)
        sizes.add(2 * group + k * steady + d)
        sizes.add(k * steady + d)
        sizes.add(group + 4 * steady + k * 4096 + d)
rng = random.Random(5)
sizes.update(rng.randrange(1, 3 * group + group // 2) for _ in range(200))
sizes.update((1, 2, 3, 4095, 4096, 4097))
problems, checked, oversized = [], 0, 0
one = {}
def schedule(n, entry):
    if (n, entry) not in one:
        one[n, entry] = swmi.host_granules(n, entry)
    return one[n, entry]
for entry in (swmi.ENTRY_PAIRS, swmi.ENTRY_PACKED, swmi.ENTRY_ONE_VS_MANY):
    for n in sorted(s for s in sizes if s > 0):
        g = swmi.host_granules(n, entry)
        checked += 1
        if min(g) < 1:
            problems.append((entry, n, "granule below one pair"))
        at, k = 0, 0
        for lo in range(0, n, group):
            gn = min(group, n - lo)
            own = []
            while k < len(g) and sum(own) < gn:
                own.append(g[k]); k += 1
            if sum(own) != gn:
                problems.append((entry, n, "group at %%d: granules sum to %%d, not %%d" %% (lo, sum(own), gn)))
                break
            if own != schedule(gn, entry):
                problems.append((entry, n, "group at %%d is not the schedule of %%d pairs" %% (lo, gn)))
        if k != len(g):
            problems.append((entry, n, "granules left over past the last group"))
        sized = [group] if n >= group else [n]
        if n > group and n %% group:
            sized.append(n %% group)
        bound = max(max(schedule(s, entry)) for s in sized)
        if max(g) != bound:
            problems.append((entry, n, "largest granule %%d, but the full and tail groups' schedules give %%d" %% (max(g), bound)))
        if n > group and max(g) > max(schedule(group, entry)):
            oversized += 1
print(json.dumps({"checked": checked, "oversized": oversized, "problems": problems[:20]}))
""" % PKG


def _run(**env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([sys.executable, "-c", CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(clean, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("env", [{}, {"SWMI_TEST_SCORE_GROUP": "1048576"},
                                 {"SWMI_TEST_SCORE_GROUP": "65536", "SWMI_HOST_MIN_GRANULE": "8192"}],
                         ids=["production_group", "group_1M", "group_64K_steady_8K"])
def test_granules_tile_every_score_group(env):
    res = _run(**env)
    assert res["problems"] == [] and res["checked"] > 300
    assert res["oversized"] > 0          # the sweep does reach tails whose granule exceeds the full group's largest


def test_packed_tail_schedule_at_the_production_group():
    """The 2-bit packed entry's balanced schedule at 2^24 + 655 359 pairs: a full group in equal granules, then a tail group
    whose last middle granule takes the rest of the 4096-pair cuts (135 167 pairs, above the full group's 131 072).  Pinned:
    score_host_batch's buffer sizing and the measured host pipeline both depend on it."""
    code = ("import sys; sys.path.insert(0, %r); import swmi; print(swmi.host_granules((1 << 24) + 655359, swmi.ENTRY_PACKED))" % PKG)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=clean)
    assert r.returncode == 0, r.stderr
    g = eval(r.stdout.strip())
    head = [32768, 98304] + [131072] * 126 + [98304, 32768]
    assert g[:len(head)] == head and sum(head) == 1 << 24
    assert g[len(head):] == [32768, 98304, 126976, 131072, 135167, 98304, 32768]
