"""Phase clocks of ONE instance alone on its compute unit, -DMPCQP_RUN_TIMING builds:  python scripts/lat_phase.py <lib.so> [backend] [iters] [tuning]
Prints cycles per ADMM iteration by phase (thread 0 of the workgroup: rhs | level 0 fwd | level 1 fwd | top | level 1 back | level 0 back | update)
and per round / per check outside the iterations (slot 9, 'boundary': everything between a round's last iteration and the next round -- termination
test, carried transition, hand-over -- and, on libraries with boundary clocks, its sections on lane 0 of every wave); per step, the wall clock of begin, the rounds, the generic checks and the loop body (output,
plant, update -- inside the round too where it carries a solve into the next step; libraries that predate that clock print no body); for the
latency round a table per WAVE as well: when lane 0 of each wave reaches each barrier of the iteration and which wave ends each phase.  The library writes its counters to stderr; this script reads them back through a pipe."""
import os, sys, re, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pympc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
backend = sys.argv[2] if len(sys.argv) > 2 else 'bcr8'
import argparse, numpy as np, torch
import bench
from pympc_amd.solver import forced_settings
dev = torch.device('cuda', 0)
tuning = int(sys.argv[4], 0) if len(sys.argv) > 4 else 0      # e.g. 0x800000 = MPCQP_TUNE_NO_CARRY
with forced_settings(backend=backend, tuning=tuning):
    sh = bench.Shard(argparse.Namespace(eps=1e-3, chunk=None), bench.WORKLOADS['cfg3'][:4], 1, 0, 1, dev, 1000, torch, None)
sh.measure('device_loop', 10, 5)
tmp = tempfile.TemporaryFile(mode='w+')
old = os.dup(2)
sh.prob.stats(reset=True)
r = sh.measure('device_loop', 20, 0)          # (its accounting reads -- and so prints and clears -- the counters once: captured)
os.dup2(tmp.fileno(), 2)
r2 = sh.measure('device_loop', 20, 0)
os.dup2(old, 2)
tmp.seek(0); txt = tmp.read()
its, rounds = r2['iters'], r2['checks']
m = [l for l in txt.splitlines() if 'iteration cycles' in l and 'total 1;' not in l][-1]
w = [l for l in txt.splitlines() if 'phase wall-clock' in l and 'admm 0' not in l][-1]
pct = [float(x) for x in re.findall(r'([0-9.]+)%', m)]
tot = float(re.search(r'total ([0-9.e+]+);', m).group(1))
outside = [float(x) for x in re.search(r't7 ([0-9.e+]+) t8 ([0-9.e+]+) t9 ([0-9.e+]+)', m).groups()]
chk = [float(x) for x in re.search(r'setup\+tail ([0-9.e+]+) rows ([0-9.e+]+) vars ([0-9.e+]+) reduce ([0-9.e+]+) decide ([0-9.e+]+)', m).groups()]
wall = [int(x) for x in re.search(r'begin (\d+) admm (\d+) check (\d+)', w).groups()]
body = re.search(r'body (\d+)', w)
names = ['rhs', 'L0fwd', 'L1fwd', 'top', 'L1back', 'L0back', 'update']
print('%s %s: %d iterations, %d rounds in 20 steps; %.0f cycles per iteration = ' % (os.path.basename(sys.argv[1]), backend, its, rounds, tot / its)
      + ' + '.join('%s %.0f' % (n, p / 100 * tot / its) for n, p in zip(names, pct)))
print('   whole admm function (thread 0): %.0f cycles per step; sum of its slots: %.0f; before the first tick %.0f' % (chk[1] / 20.0, (tot + sum(outside)) / 20.0, chk[2] / 20.0))
print('   per round: load %.0f  owner regs %.0f  boundary %.0f cycles;  per check: setup+tail %.0f vars %.0f reduce %.0f decide %.0f cycles;  wall (10 ns ticks) per step: begin %.0f admm %.0f check %.0f'
      % tuple([o / rounds for o in outside] + [chk[0] / rounds, chk[2] / rounds, chk[3] / rounds, chk[4] / rounds] + [x / 20.0 for x in wall]))
bl = [l for l in txt.splitlines() if l.startswith('boundary cycles')]
if bl:                                        # (libraries with boundary clocks, mpcqp_layout.h BTICK: the sections of slot 9, lane 0 of each wave, cycles per round)
    g = re.findall(r' s\d((?: \d+)+)', bl[-1])
    arr = np.array([[int(x) for x in s.split()] for s in g], dtype=float) / rounds       # [section, wave]
    secs = ['check entry', 'exchanges', 'rows+vars', 'reduction', 'solved tail', 'check stage 2', 'plant', 'update+types', 'hand-over', 'other verdict']
    print('   boundary, cycles per round by section (mean over the waves / slowest wave): '
          + '  '.join('%s %.0f/%.0f' % (n, r.mean(), r.max()) for n, r in zip(secs, arr)) + '  | sum of the means %.0f' % arr.mean(axis=1).sum())
wl = [l for l in txt.splitlines() if l.startswith('wave barrier cycles')]
if wl:                                        # (libraries with per-wave clocks: when lane 0 of each wave reaches each barrier of the iteration, cycles since the wave's start)
    g = re.findall(r' b\d((?: \d+)+)', wl[-1])
    arr = np.array([[int(x) for x in s.split()] for s in g], dtype=float) / its          # [barrier, wave]
    if arr.any():
        nwv = max(w for w in range(arr.shape[1]) if arr[:, w].any()) + 1
        bars = ['rhs+L0fwd', 'L1fwd', 'top', 'back', 'update'] if arr[3].any() else ['b0', 'b1', 'b2', 'b3', 'b4']
        print('   per wave: arrival at the barrier that ends each phase, cycles since the iteration started (* = last to arrive) | work in the phase since the previous arrival of the last wave')
        print('   %-10s' % 'phase' + ''.join('%8s' % ('w%d' % w) for w in range(nwv)) + ' |' + ''.join('%8s' % ('w%d' % w) for w in range(nwv)))
        prev = 0.0
        for k, nm in enumerate(bars):
            row = arr[k, :nwv]; last = row.max()
            print('   %-10s' % nm + ''.join('%7.0f%s' % (x, '*' if x == last else ' ') for x in row) + ' |' + ''.join('%8.0f' % (x - prev) for x in row))
            prev = last
print('   per step: cycles of the admm function outside the iterations %.0f;  wall (10 ns ticks): begin %.0f%s  begin+check+body %s'
      % ((chk[1] - tot) / 20.0, wall[0] / 20.0, ('  body %.0f' % (int(body.group(1)) / 20.0)) if body else '',
         ('%.0f' % ((wall[0] + wall[2] + int(body.group(1))) / 20.0)) if body else 'n/a'))
