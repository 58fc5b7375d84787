"""Registers, spills, scratch and LDS of the kernels of a built library (the code objects' metadata notes):

    python tools/kernel_resources.py [library.so] [kernel-name-substring]
"""
import contextlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
NOTE_KEYS = ('agpr_count', 'vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
             'group_segment_fixed_size', 'name')


@contextlib.contextmanager
def code_objects(path):
    """paths of the gfx950 code objects embedded in a built library (extracted into a directory that lives as long as the block)"""
    tmp = tempfile.mkdtemp()
    try:
        local = os.path.join(tmp, os.path.basename(path))
        shutil.copy(path, local)
        subprocess.run([f'{LLVM}/llvm-objdump', '--offloading', local], check=True, cwd=tmp, capture_output=True)
        yield [os.path.join(tmp, obj) for obj in sorted(os.listdir(tmp)) if 'gfx950' in obj]
    finally:
        shutil.rmtree(tmp)


def notes(obj):
    """the kernels' entries of one code object's metadata note"""
    text = subprocess.run([f'{LLVM}/llvm-readelf', '--notes', obj], check=True, capture_output=True, text=True).stdout
    for block in re.split(r'\n\s*- \.agpr_count:', text)[1:]:
        block = '.agpr_count:' + block
        entry = {}
        for key in NOTE_KEYS:
            m = re.search(r'\.' + key + r':\s*(\S+)', block)
            if m:
                entry[key] = m.group(1)
        yield entry


def kernels(path):
    with code_objects(path) as objs:
        for obj in objs:
            yield from notes(obj)


def demangle(names):
    """short kernel names, as the tools print them: demangled, without the anonymous namespace and the argument list"""
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return [re.sub(r'\(anonymous namespace\)::', '', d).split('(')[0].replace('void ', '') for d in out[:len(names)]]


if __name__ == '__main__':
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'ppgs_amd', 'libppgs_amd.so')
    want = sys.argv[2] if len(sys.argv) > 2 else ''
    found = list(kernels(lib))
    for k, name in zip(found, demangle([k.get('name', '?') for k in found])):
        if want in name:
            print(f"{name[:70]:70s} vgpr {k.get('vgpr_count'):>4} agpr {k.get('agpr_count'):>4} sgpr {k.get('sgpr_count'):>4} "
                  f"spill v {k.get('vgpr_spill_count'):>4} s {k.get('sgpr_spill_count'):>3} scratch {k.get('private_segment_fixed_size'):>5} lds {k.get('group_segment_fixed_size'):>6}")
