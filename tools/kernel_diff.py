"""Kernel-by-kernel comparison of two builds of the library: what a refactor that moves kernels between units must
leave as it was.

    python tools/kernel_diff.py old.so new.so

For every kernel (demangled name) of the gfx950 code objects of either library, one of
    equal       same code bytes, same kernel descriptor, same metadata (registers, spills, scratch, LDS)
    DIFFERENT   with what differs
    only in old / only in new
The code is the bytes of the kernel's function symbol; the descriptor is the 64 bytes of `<kernel>.kd` without its
kernel_code_entry_byte_offset (bytes 16..23: the distance from the descriptor to the code, which depends on what else
is in the code object and on nothing in the kernel).  Exit status 1 if a kernel differs or exists only in the new
library.
"""
import hashlib
import struct
import sys

from kernel_resources import NOTE_KEYS, code_objects, demangle, notes


def symbols(obj):
    """{symbol: its bytes} for the sized symbols of an ELF64 little-endian object"""
    data = open(obj, 'rb').read()
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    # (type, address, file offset, size, link, entry size) of every section
    secs = [struct.unpack_from('<4xI8xQQQI12xQ', data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for kind, _, off, size, link, entsize in secs:
        if kind != 2:       # SHT_SYMTAB
            continue
        strtab = secs[link][2]
        for at in range(off, off + size, entsize):
            name, _, _, shndx, value, length = struct.unpack_from('<IBBHQQ', data, at)
            if not length or not 0 < shndx < shnum or secs[shndx][0] == 8:      # (SHT_NOBITS: nothing in the file)
                continue
            start = secs[shndx][2] + value - secs[shndx][1]
            out[data[strtab + name:data.index(b'\0', strtab + name)].decode()] = data[start:start + length]
    return out


def kernels(path):
    """{demangled name: (code, descriptor, metadata)} of a built library"""
    found = {}
    with code_objects(path) as objs:
        for obj in objs:
            syms = symbols(obj)
            for note in notes(obj):
                name = note['name']
                kd = syms[name + '.kd']
                found[name] = (syms[name], kd[:16] + kd[24:], {k: note.get(k) for k in NOTE_KEYS if k != 'name'})
    short = dict(zip(demangle(list(found)), found.values()))
    assert len(short) == len(found), 'two kernels with one short name'
    return short


def sha16(path):
    with open(path, 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    print(f'# old {old_path}  library_sha16={sha16(old_path)}  {len(old)} kernels')
    print(f'# new {new_path}  library_sha16={sha16(new_path)}  {len(new)} kernels')
    count = dict.fromkeys(('equal', 'DIFFERENT', 'only in old', 'only in new'), 0)
    for name in sorted(set(old) | set(new)):
        if name not in new or name not in old:
            verdict = 'only in old' if name in old else 'only in new'
        else:
            (code_a, kd_a, meta_a), (code_b, kd_b, meta_b) = old[name], new[name]
            what = [f'code ({len(code_a)} / {len(code_b)} bytes)'] * (code_a != code_b) + ['descriptor'] * (kd_a != kd_b)
            what += [f'{k} {meta_a[k]} / {meta_b[k]}' for k in meta_a if meta_a[k] != meta_b[k]]
            verdict = 'DIFFERENT: ' + ', '.join(what) if what else 'equal'
        count[verdict.split(':')[0]] += 1
        print(f'{verdict:12s} {name}')
    print('# ' + ', '.join(f'{v} {k}' for k, v in count.items()))
    return 1 if count['DIFFERENT'] or count['only in new'] else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
