"""Which LDS instruction forms does the compiler emit in the phases of the latency round's iteration?  CPU only (hipcc cross-compiles).
    python scripts/lds_forms.py [--inst 16,true,12,4,231] [--asm w8.s] [--keep w8.s] [extra compiler flags, e.g. -DMPCQP_RUN_TIMING]
Compiles pympc_amd/csrc/mpcqp_w8.hip to gfx950 assembly with the flags of csrc/build.sh (or reads --asm), takes w8::run_admm_phase<inst>, finds the
iteration loop of admm_latw (the smallest loop of the function that holds both MFMAs and barriers) and walks its control-flow graph from the loop
header: an instruction belongs to the phase given by the number of s_barrier passed on the way to it (the compiler duplicates a barrier into the
eight per-wave cases of LATW_DISPATCH, so the text order alone does not say).  Per phase it prints static counts -- summed over the per-wave cases,
i.e. what the compute unit's LDS sees per iteration; instructions in front of a wave switch run on all eight waves and count once --
of ds_read_b64 | ds_read2_b64 + ds_read2st64_b64 | ds_read_b128 | ds_write_b64 | ds_write2_b64 + ds_write2st64_b64 | other ds_* | v_mfma*, and the LDS-array
cycles these forms cost by MI355X's rates (ds_read_b64 2, ds_read2_b64 8, ds_read_b128 4, ds_write_b64 4, ds_write2_b64 8 per wave instruction).
    python scripts/lds_forms.py --boundary [--inst ...] [--asm w8.s]
prints instead the static counts of the boundary between two rounds (w8::latw_check<NXT,NUT,NST>, see boundary() below)."""
import argparse, collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pympc_amd', 'csrc')
COLS = ['ds_read_b64', 'ds_read2_b64', 'ds_read_b128', 'ds_write_b64', 'ds_write2_b64', 'ds_other', 'mfma']
CYCLES = {'ds_read_b64': 2, 'ds_read2_b64': 8, 'ds_read_b128': 4, 'ds_write_b64': 4, 'ds_write2_b64': 8}
FUSED = ['rhs + level 0 forward', 'level 1 forward', 'top', 'back substitution', 'owner update', 'loop tail']
UNFUSED = ['rhs', 'level 0 forward', 'level 1 forward', 'top', 'level 1 back', 'level 0 back', 'owner update', 'loop tail']


def build_flags():
    """FLAGS of csrc/build.sh, without the resource remarks."""
    for line in open(os.path.join(CSRC, 'build.sh')):
        m = re.match(r'FLAGS="(.*)"', line.strip())
        if m:
            return [f for f in m.group(1).split() if not f.startswith('-Rpass')]
    raise SystemExit('no FLAGS line in build.sh')


def compile_asm(out, extra):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc] + build_flags() + extra + ['--cuda-device-only', '-S', 'mpcqp_w8.hip', '-o', out], cwd=CSRC)


def classify(op):
    if op.startswith('v_mfma'): return 'mfma'
    if not op.startswith('ds_'): return None
    if op == 'ds_read_b64': return 'ds_read_b64'
    if op in ('ds_read2_b64', 'ds_read2st64_b64'): return 'ds_read2_b64'
    if op == 'ds_read_b128': return 'ds_read_b128'
    if op == 'ds_write_b64': return 'ds_write_b64'
    if op in ('ds_write2_b64', 'ds_write2st64_b64'): return 'ds_write2_b64'
    return 'ds_other'


def function_blocks(lines, name):
    """Basic blocks of one function: list of (label, [opcodes], [successor labels], falls_through)."""
    start = next((i for i, l in enumerate(lines) if l.startswith(name) and l.split(':')[0].startswith(name) and ':' in l), None)
    if start is None:
        raise SystemExit('no function %s* in the assembly' % name)
    blocks, cur = [], ['<entry>', [], [], True]
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith('.Lfunc_end'): break
        m = re.match(r'(\.LBB\d+_\d+):', s)
        if m:
            blocks.append(cur); cur = [m.group(1), [], [], True]
            continue
        if not s or s[0] in '.;': continue
        tok = s.split()
        op = tok[0]
        if not cur[3]:                                    # (code behind an unconditional branch without a label: unreachable)
            continue
        cur[1].append(op)
        if op.startswith('s_cbranch'):
            cur[2].append(tok[1])
        elif op == 's_branch':
            cur[2].append(tok[1]); cur[3] = False
        elif op in ('s_endpgm', 's_setpc_b64'):
            cur[3] = False
    blocks.append(cur)
    return blocks


def iteration_loop(blocks):
    """(header index, set of block indices) of the smallest natural loop that holds MFMAs and barriers."""
    idx = {b[0]: i for i, b in enumerate(blocks)}
    succ = [[idx[t] for t in b[2] if t in idx] + ([i + 1] if b[3] and i + 1 < len(blocks) else []) for i, b in enumerate(blocks)]
    pred = collections.defaultdict(list)
    for i, ss in enumerate(succ):
        for j in ss: pred[j].append(i)
    loops = {}
    for u, ss in enumerate(succ):
        for h in ss:
            if h > u: continue                           # a back edge in layout order
            body, stack = {h, u}, [u]
            while stack:
                x = stack.pop()
                if x == h: continue
                for p in pred[x]:
                    if p not in body: body.add(p); stack.append(p)
            loops.setdefault(h, set()).update(body)
    best = None
    for h, body in loops.items():
        ops = [op for i in body for op in blocks[i][1]]
        if any(o.startswith('v_mfma') for o in ops) and 's_barrier' in ops:
            if best is None or len(ops) < best[2]: best = (h, body, len(ops))
    if best is None:
        raise SystemExit('no loop with MFMAs and barriers')
    return best[0], best[1], succ


def phases(blocks, header, body, succ):
    """Counts per phase (barriers passed since the loop header)."""
    seen, work = {}, [(header, 0)]
    counts = collections.defaultdict(lambda: collections.Counter())
    clash = nbar = 0
    while work:
        b, k = work.pop()
        if b in seen:
            clash += seen[b] != k
            continue
        seen[b] = k
        for op in blocks[b][1]:
            if op == 's_barrier': k += 1; continue
            c = classify(op)
            if c: counts[k][c] += 1
        nbar = max(nbar, k)
        for s in succ[b]:
            if s in body and s != header: work.append((s, k))
    return counts, clash, nbar


def function_text(lines, name):
    """Instruction lines (opcode and operands) of the first function whose symbol starts with name; None if there is none."""
    start = next((i for i, l in enumerate(lines) if l.startswith(name) and ':' in l), None)
    if start is None:
        return None
    out = []
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith('.Lfunc_end'): break
        if s and s[0] not in '.;': out.append(s)
    return out


def boundary(lines, nxt, nut, mode):
    """The boundary between two rounds: w8::latw_check<NXT,NUT,NST> -- termination test and, inline, the carried transition -- and, in trees where
    the carry is a call of its own, w8::latw_carry<...> beside it.  Static counts in text order, not weighted by how often a path runs."""
    nst = int(mode) % 100
    tot = collections.Counter()
    for fn in ('latw_check', 'latw_carry'):
        text = function_text(lines, '_ZN2w8%d%sILi%sELi%sELi%dEEE' % (len(fn), fn, nxt, nut, nst))
        if text is None:
            print('w8::%s<%s,%s,%d>: not a function of its own' % (fn, nxt, nut, nst))
            continue
        ops = [t.split()[0] for t in text]
        first = ops.index('s_barrier') if 's_barrier' in ops else len(ops)
        # (inst_of masks the map entry with PERM_INST_MASK: one 'and' with that literal per load of the map, vector or scalar)
        c = collections.Counter({
            'vector loads of the instance map': sum(o == 'v_and_b32' and '0xffffff' in t for o, t in zip(ops, text)),
            'scalar loads of the instance map': sum(o == 's_and_b32' and '0xffffff' in t for o, t in zip(ops, text)),
            's_waitcnt vmcnt(0) in front of the first barrier': sum(o == 's_waitcnt' and 'vmcnt(0)' in t for o, t in zip(ops[:first], text[:first])),
            'barriers': ops.count('s_barrier'),
            'flat_load': sum(o.startswith('flat_load') for o in ops),
            'global_load': sum(o.startswith('global_load') for o in ops),
            's_load': sum(o.startswith('s_load') for o in ops),
            's_waitcnt': ops.count('s_waitcnt'),
            'scratch / buffer accesses': sum(o.startswith('scratch_') or o.startswith('buffer_') for o in ops),
            'instructions': len(ops)})
        tot.update(c)
        print('w8::%s<%s,%s,%d>:' % (fn, nxt, nut, nst) + ''.join('\n    %-50s %5d' % kv for kv in c.items()))
    print('together:' + ''.join('\n    %-50s %5d' % kv for kv in tot.items()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--boundary', action='store_true', help='instead: static counts of the boundary between two rounds (latw_check with the carry in it)')
    ap.add_argument('--inst', default='16,true,12,4,231', help='template arguments NB,LDSSTATE,NXT,NUT,MODE of run_admm_phase')
    ap.add_argument('--asm', help='read this assembly instead of compiling')
    ap.add_argument('--keep', help='keep the compiled assembly here')
    args, extra = ap.parse_known_args()
    nb, lds, nxt, nut, mode = [a.strip() for a in args.inst.split(',')]
    name = '_ZN2w814run_admm_phaseILi%sELb%dELi%sELi%sELi%sEEE' % (nb, lds in ('true', '1'), nxt, nut, mode)
    if args.asm:
        path = args.asm
    else:
        path = args.keep or os.path.join(tempfile.mkdtemp(), 'w8.s')
        compile_asm(os.path.abspath(path), extra)
    lines = open(path).read().splitlines()
    if args.boundary:
        return boundary(lines, nxt, nut, mode)
    blocks = function_blocks(lines, name)
    header, body, succ = iteration_loop(blocks)
    counts, clash, nbar = phases(blocks, header, body, succ)
    n = max(counts) + 1
    # (the last barrier usually sits right in front of the back edge: no 'loop tail' then)
    names = FUSED if n in (len(FUSED) - 1, len(FUSED)) else UNFUSED if n in (len(UNFUSED) - 1, len(UNFUSED)) else ['phase %d' % i for i in range(n)]
    print('w8::run_admm_phase<%s>: iteration loop at %s, %d blocks, %d barriers per iteration%s'
          % (args.inst, blocks[header][0], len(body), nbar, '' if not clash else '  (WARNING: %d blocks reached with different barrier counts)' % clash))
    print('%-24s' % 'phase' + ''.join('%15s' % c for c in COLS) + '%12s' % 'LDS cycles')
    tot = collections.Counter()
    for k in range(n):
        c = counts[k]; tot.update(c)
        print('%-24s' % names[k] + ''.join('%15d' % c[x] for x in COLS) + '%12d' % sum(c[x] * w for x, w in CYCLES.items()))
    print('%-24s' % 'iteration' + ''.join('%15d' % tot[x] for x in COLS) + '%12d' % sum(tot[x] * w for x, w in CYCLES.items()))


if __name__ == '__main__':
    main()
