"""One line per kernel of a built library or object file: a digest of the kernel's instruction bytes and its demangled name --
the repeatable form of "this change leaves the device code byte-identical" (a move between translation units, a host-only change).

    python tools/kernel_isa_digest.py [lib.so | file.o] [name-substring]  >  a.txt        # then diff the two builds' lists

The instruction bytes are those of the kernel's own symbol in the gfx950 code object (tools/kernel_resources.py finds the code
objects and names the kernels).  A device function the compiler left out of line is a symbol of its own and is listed too, marked
`func`: a kernel that calls one holds a pc-relative offset to it, so its digest then depends on where the linker put the two.
"""
import hashlib
import os
import struct
import subprocess
import sys

from kernel_resources import code_objects, notes


def functions(elf):
    """(mangled name, instruction bytes) of every function symbol the code object defines"""
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', elf, 0x3A)
    sec = [struct.unpack_from('<IIQQQQII', elf, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr off size link info
    symtabs = [s for s in sec if s[1] == 2] or [s for s in sec if s[1] == 11]       # .symtab, else .dynsym
    for tab in symtabs:
        stroff = sec[tab[6]][4]
        for p in range(tab[4], tab[4] + tab[5], 24):
            name_off, info, _, shndx, value, size = struct.unpack_from('<IBBHQQ', elf, p)
            if info & 15 != 2 or shndx == 0 or shndx >= shnum or size == 0:       # STT_FUNC, defined
                continue
            at = sec[shndx][4] + value - sec[shndx][3]
            yield elf[stroff + name_off: elf.index(b'\0', stroff + name_off)].decode(), elf[at:at + size]


def digests(path):
    """{mangled name: (is_kernel, sha256 of the instruction bytes, byte count)}; a name two code objects define with different
    bytes keeps every digest, joined by '+'"""
    out = {}
    for co in code_objects(open(path, 'rb').read()):
        kernels = {k['.name'] for md in notes(co) for k in md.get('amdhsa.kernels', [])}
        for name, code in functions(co):
            d = hashlib.sha256(code).hexdigest()[:16]
            if name in out and d not in out[name][1].split('+'):
                d = out[name][1] + '+' + d
            out[name] = (name in kernels, d, len(code))
    return out


if __name__ == '__main__':
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), '..', 'aspire_amd', 'lib', 'libaspire_hip.so')
    sub = sys.argv[2] if len(sys.argv) > 2 else ''
    found = digests(lib)
    names = sorted(found)
    plain = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    for name, shown in sorted(zip(names, plain), key=lambda t: t[1]):
        is_kernel, d, n = found[name]
        if sub in shown:
            print(f"{d} {n:7d} B {'kernel' if is_kernel else 'func  '} {shown}")
