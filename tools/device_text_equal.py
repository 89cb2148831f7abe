"""Is the device code of two builds the same?  Compares, object file by object file, the .text section of the gfx950 code
object inside the offload bundle -- the check of a host-only change (the ELF as a whole carries per-compilation data outside
.text, so it differs between any two compilations).

    python tools/device_text_equal.py build_a/obj build_b/obj      # directories of *.hip.o from __graft_entry__.build()

Prints a markdown table (file, .text bytes, equal / NOT EQUAL); exit status 1 if any file differs.
"""
import os
import struct
import sys

from kernel_resources import code_objects


def text_section(elf):
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', elf, 0x3A)
    stroff, = struct.unpack_from('<Q', elf, shoff + shstrndx * shentsize + 0x18)
    for i in range(shnum):
        sh = shoff + i * shentsize
        name_off, = struct.unpack_from('<I', elf, sh)
        off, size = struct.unpack_from('<QQ', elf, sh + 0x18)
        name = elf[stroff + name_off: elf.index(b'\0', stroff + name_off)]
        if name == b'.text':
            return elf[off:off + size]
    return b''


def device_text(path):
    return [text_section(co) for co in code_objects(open(path, 'rb').read())]


if __name__ == '__main__':
    dir_a, dir_b = sys.argv[1:3]
    names = sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b)))
    differ = 0
    print('| object | gfx950 .text bytes | device code |')
    print('|---|---|---|')
    for n in (n for n in names if n.endswith('.o')):
        pa, pb = os.path.join(dir_a, n), os.path.join(dir_b, n)
        ta = device_text(pa) if os.path.exists(pa) else None
        tb = device_text(pb) if os.path.exists(pb) else None
        same = ta is not None and ta == tb
        differ += not same
        size = sum(len(t) for t in tb) if tb is not None else 0
        print(f"| {n} | {size} | {'equal' if same else 'NOT EQUAL'} |")
    sys.exit(1 if differ else 0)
