"""What the compiler made of the tile loops of csrc/policy_mfma.hip: compiles the file for gfx950 with the Makefile's flags plus
--cuda-device-only -S and prints one row per kernel and tile loop:

  vgpr      .amdhsa_next_free_vgpr of the kernel descriptor
  priv      .amdhsa_private_segment_fixed_size (bytes; anything but 0 is a spill or a run-time indexed array)
  mfma      v_mfma instructions in the loop (a loop unrolled over two input buffers holds two tiles)
  vm0_head  s_waitcnt with vmcnt(0) between the loop's first load from memory (the prefetch issue) and its first v_mfma: a full wait right behind
            the prefetch.  A wait at the top of the trip, ahead of the prefetch, is the wait for loads issued a tile earlier and is not counted here
  vm0_loop  s_waitcnt with vmcnt(0) anywhere in the loop
  lines     instructions in the loop

A tile loop is an outermost loop (by the compiler's own block comments) that contains a v_mfma; a kernel with two bodies (the PPO-KL gate, the VJP form
of the gradient kernel) has one row per body, in text order.  The tool reads descriptors, block comments, v_mfma, s_waitcnt and the mnemonics of loads only.

  python tools/policy_loop_audit.py                   # compile me-trpo_amd/csrc/policy_mfma.hip and print the table
  python tools/policy_loop_audit.py --asm listing.s   # a listing made elsewhere
  python tools/policy_loop_audit.py --against old.s   # two listings side by side (old | new)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'me-trpo_amd', 'csrc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I../../include', '-I.', '-Wall', '-Wno-unused-function']      # csrc/Makefile CXXFLAGS

_BLOCK = re.compile(r'^(?:(\.LBB\d+_\d+):|; (%bb\.\d+):)')                     # a basic block: its label, or the comment of a fall-through block
_SELF1 = re.compile(r'=>This (?:Inner )?Loop Header: Depth=1\b')
_HEADER1 = re.compile(r'in Loop: Header=(BB\d+_\d+) Depth=1\b')
_PARENT1 = re.compile(r'Parent Loop (BB\d+_\d+) Depth=1\b')
_VM0 = re.compile(r'^\s+s_waitcnt\b.*\bvmcnt\(0\)')
_KERNEL = re.compile(r'^\s+\.amdhsa_kernel\s+(\S+)')
_FIELD = re.compile(r'^\s+\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\d+)')
_LOAD = re.compile(r'^\s+(?:global|buffer|flat)_load_')
_INSN = re.compile(r'^\s+[a-z]\w*')
_TEMPLATE = re.compile(r'k_policy_mfmaILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E')


def compile_listing(src=None, hipcc=None, extra=()):
    """-> the gfx950 text of policy_mfma.hip (device side only)."""
    hipcc = hipcc or os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    src = src or os.path.join(CSRC, 'policy_mfma.hip')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'policy_mfma.s')
        subprocess.check_call([hipcc] + FLAGS + list(extra) + ['--cuda-device-only', '-S', os.path.abspath(src), '-o', out], cwd=CSRC)
        with open(out) as f:
            return f.read()


def short_name(sym):
    m = _TEMPLATE.search(sym)
    return 'k_policy_mfma<%s,%s,%s,%s>' % m.groups() if m else sym


def parse(text):
    """-> [dict(kernel, vgpr, priv, loops=[dict(mfma, vm0_head, vm0_loop, lines)])] in text order."""
    lines = text.splitlines()
    desc = {}                                               # symbol -> {field: value}
    cur = None
    for ln in lines:
        m = _KERNEL.match(ln)
        if m:
            cur = desc.setdefault(m.group(1), {})
            continue
        if ln.strip() == '.end_amdhsa_kernel':
            cur = None
        m = _FIELD.match(ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    out = []
    for sym, d in desc.items():
        try:
            start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ':'))
        except StopIteration:
            continue
        end = next((i for i in range(start + 1, len(lines)) if lines[i].startswith('.Lfunc_end') or lines[i].lstrip().startswith('.end_amdhsa_kernel')
                    or lines[i].lstrip().startswith('.amdhsa_kernel')), len(lines))
        out.append(dict(kernel=short_name(sym), vgpr=d.get('next_free_vgpr', -1), priv=d.get('private_segment_fixed_size', -1),
                        loops=tile_loops(lines[start:end])))
    return out


def tile_loops(body):
    """Rows of the outermost loops of one function that hold a v_mfma, in text order.  Loop membership comes from the block comments the compiler
    writes ('=>This Inner Loop Header: Depth=1', 'in Loop: Header=BB0_38 Depth=1', 'Parent Loop BB0_38 Depth=1'), not from branch
    directions: block placement moves cold blocks of the function between a loop's blocks."""
    loops, order, cur = {}, [], None                        # depth-1 header label -> lines of its blocks, in text order
    i = 0
    while i < len(body):
        ln = body[i]
        m = _BLOCK.match(ln)
        if m:
            label, note = m.group(1) or m.group(2), ln
            j = i + 1
            while j < len(body) and body[j].lstrip().startswith(';') and not _BLOCK.match(body[j]):       # continuation comments of the block header
                note += body[j]; j += 1
            cur = None
            top = _PARENT1.search(note) or _HEADER1.search(note)
            if top:
                cur = top.group(1)
            elif _SELF1.search(note) and m.group(1):
                cur = label.lstrip('.L')
            if cur is not None and cur not in loops:
                loops[cur] = []; order.append(cur)
        elif cur is not None:
            loops[cur].append(ln)
        i += 1
    rows = []
    for h in order:
        seg = loops[h]
        if not any('v_mfma' in ln for ln in seg):
            continue
        first = next(i for i, ln in enumerate(seg) if 'v_mfma' in ln)
        load = next((i for i, ln in enumerate(seg[:first]) if _LOAD.match(ln)), first)
        rows.append(dict(mfma=sum('v_mfma' in ln for ln in seg), vm0_head=sum(bool(_VM0.match(ln)) for ln in seg[load:first]),
                         vm0_loop=sum(bool(_VM0.match(ln)) for ln in seg), lines=sum(bool(_INSN.match(ln)) for ln in seg)))
    return rows


COLS = ('vgpr', 'priv', 'mfma', 'vm0_head', 'vm0_loop', 'lines')


def rows_of(parsed):
    """-> {(kernel, loop index): {column: value}}; a kernel without a tile loop has one row with index 0 and no loop columns."""
    out = {}
    for k in parsed:
        for j, lp in enumerate(k['loops'] or [{}]):
            r = dict(vgpr=k['vgpr'], priv=k['priv']); r.update(lp)
            out[k['kernel'], j] = r
    return out


def table(new, old=None):
    rn, ro = rows_of(new), rows_of(old) if old is not None else None
    keys = list(rn) + [k for k in (ro or {}) if k not in rn]
    head = '%-34s %4s' % ('kernel', 'loop') + ''.join(' %17s' % c if ro is not None else ' %8s' % c for c in COLS)
    out = [head]
    for key in keys:
        cells = []
        for c in COLS:
            n = rn.get(key, {}).get(c, '-')
            cells.append(' %17s' % ('%s | %s' % (ro.get(key, {}).get(c, '-'), n)) if ro is not None else ' %8s' % n)
        out.append('%-34s %4d' % key + ''.join(cells))
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--asm', help='audit this listing instead of compiling')
    ap.add_argument('--against', help='an older listing: print old | new in every column')
    ap.add_argument('--src', help='another source file than csrc/policy_mfma.hip')
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else compile_listing(a.src)
    old = parse(open(a.against).read()) if a.against else None
    print(table(parse(text), old))
    return 0


if __name__ == '__main__':
    sys.exit(main())
