#!/usr/bin/env python3
"""Compare two builds' device code kernel by kernel (no GPU needed).

    for f in video_features_amd/ops/csrc/*.hip; do
      hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only \\
            -S $f -o DIR/$(basename $f .hip).s
    done                      # once per build, then
    python tools/diff_device_asm.py DIR_A DIR_B

Each .s file is split at its kernel symbols (``.type SYM,@function`` up to
the register summary).  Comments, blank lines and the ``__hip_cuid_*`` lines
(a hash of the source path) are dropped; the function-local label numbers
(``.LBB<n>_``, ``.Lfunc_end<n>``), which count kernels in instantiation
order, and the kernel's own symbol are blanked.  Kernels pair by symbol.  A
kernel left without a partner pairs with one of the other side's leftovers
of the same file whose text is identical and is listed as renamed (the
mangled name of a kernel changes when a parameter type changes namespace).
Prints every kernel whose text differs or that stays unpaired; exit status 1
if there is any.  It compares text, nothing else."""
import re
import sys
from pathlib import Path

KERNEL = re.compile(r'^\t\.type\t(\S+),@function$', re.M)


def kernels(path: Path) -> dict:
    """{symbol: normalised text} of the kernels of one .s file."""
    if not path.exists():
        return {}
    text = path.read_text()
    out = {}
    for m in KERNEL.finditer(text):
        sym = m.group(1)
        body = text[m.start():text.index('\t.section\t.AMDGPU.csdata',
                                         m.start())]
        body = re.sub(r';.*', '', body.replace(sym, '<kernel>'))
        body = re.sub(r'\.LBB\d+_', '.LBB_', body)
        body = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', body)
        lines = [ln.rstrip() for ln in body.split('\n')]
        out[sym] = '\n'.join(ln for ln in lines
                             if ln and '__hip_cuid_' not in ln)
    return out


def main(dir_a: str, dir_b: str) -> int:
    a, b = Path(dir_a), Path(dir_b)
    total = renamed = bad = 0
    for stem in sorted({p.stem for d in (a, b) for p in d.glob('*.s')}):
        ka, kb = kernels(a / f'{stem}.s'), kernels(b / f'{stem}.s')
        total += len(ka.keys() | kb.keys())
        for sym in sorted(ka.keys() & kb.keys()):
            if ka[sym] != kb[sym]:
                print(f'{stem}: differs: {sym}')
                bad += 1
        only_b = {s: kb[s] for s in sorted(kb.keys() - ka.keys())}
        for sym in sorted(ka.keys() - kb.keys()):
            twin = next((s for s, t in only_b.items() if t == ka[sym]), None)
            if twin is None:
                print(f'{stem}: only in {dir_a}: {sym}')
                bad += 1
            else:
                print(f'{stem}: renamed, same text: {sym} -> {twin}')
                del only_b[twin]
                renamed += 1
                total -= 1
        for sym in only_b:
            print(f'{stem}: only in {dir_b}: {sym}')
            bad += 1
    print(f'{total} kernels: {total - renamed - bad} identical, {renamed} '
          f'renamed with identical text, {bad} differ or are unpaired')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
