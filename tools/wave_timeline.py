"""Per-wave timeline of step launches (development aid): start skew, durations and the tail of the 1024 waves.

usage (GPU box):  python tools/wave_timeline.py [launches]
Uses the -DORR_PHASE_TIMERS build (see tools/phase_cycles.py).  The kernel ends when its slowest wave ends, so what matters is the
latest end, not the mean: the report splits the waves of each launch by whether one of their robots finished an episode (reset inside
the launch) and shows which group sets the end of the launch.
"""
import sys

import numpy as np

import dev_build

n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
L = dev_build.load(*dev_build.PHASE_TIMERS)
env, act = dev_build.laikago_env(4096)
W = 1024
dev_build.wave_rows(L, W)          # allocate: the launches from here on are recorded
for _ in range(300):
    env.step(act)
rows = []
for _ in range(n):
    env.step(act)
    a = dev_build.wave_rows(L, W)
    t0 = a[:, 0].min()
    start, end = (a[:, 0] - t0) / 100.0, (a[:, 1] - t0) / 100.0      # microseconds (100 MHz realtime counter)
    reset = dev_build.decode_slot(a)[0] != 0
    last = int(np.argmax(end))
    rows.append((start.max(), end.max(), (end - start).mean(), (end - start)[reset].mean() if reset.any() else np.nan,
                 (end - start)[~reset].mean(), end[~reset].max(), end[reset].max() if reset.any() else np.nan, reset.sum(), bool(reset[last]),
                 a[:, 2].mean(), a[reset, 2].mean() if reset.any() else np.nan, a[~reset, 2].mean(), a[~reset, 2].max()))
r = np.array(rows, dtype=np.float64)
names = ["latest wave start (us)", "latest wave end = launch length (us)", "mean wave duration (us)", "  waves with a reset (us)",
         "  waves without (us)", "latest end among waves without a reset (us)", "latest end among waves with a reset (us)", "waves with a reset",
         "launches whose last wave had a reset (fraction)", "mean shader cycles per wave", "  waves with a reset", "  waves without",
         "  max over waves without"]
for k, nm in enumerate(names):
    print("%-55s %10.2f" % (nm, np.nanmean(r[:, k])))
