"""The structural rule of libomgx.so's translation units ("Handle: ownership and the instance table"), checked on the
objects of the build directory without a device: every kernel of the gfx950 code objects is compiled in exactly one unit, the host
unit (omgx.hip) holds no ipm_* kernel instance, and the set of kernels is the committed one (tests/golden/kernel_names.txt: an
instance lost or added by a later change shows as a diff to that file).  Symbol names only: nothing is disassembled."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'omg-tools_amd', 'csrc', 'build')
LLVM = '/opt/rocm/lib/llvm/bin'
TOOLS = [os.path.join(LLVM, t) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf')]
IPM = ('ipm_solve_kernel', 'ipm_eval_kernel', 'ipm_rollout_kernel', 'ipm_prepare_kernel')


def _kernels_of(obj, tmp):
    """names of the kernels (symbols with a kernel descriptor) in the gfx950 code object bundled into a host object"""
    fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, 'co.o')
    subprocess.check_call([TOOLS[0], '-O', 'binary', '--only-section=.hip_fatbin', obj, fat])
    subprocess.check_call([TOOLS[1], '--unbundle', '--type=o', '--input=' + fat, '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co])
    names = set()      # (a code object lists a kernel in .dynsym and in .symtab)
    for line in subprocess.check_output([TOOLS[2], '-sW', '--demangle', co], universal_newlines=True).splitlines():
        f = line.split(None, 7)
        if len(f) == 8 and f[3] == 'OBJECT' and f[7].rstrip().endswith('.kd)'):
            m = re.match(r'(?:void )?((?:\(anonymous namespace\)::)?[^(]+)\(', f[7])
            assert m, f[7]
            names.add(m.group(1))
    return sorted(names)


@pytest.fixture(scope='module')
def units(tmp_path_factory):
    # the object of every translation unit of the source directory (not whatever lies in build/: an object left behind by a unit
    # that no longer exists is not part of the library)
    sources = sorted(glob.glob(os.path.join(os.path.dirname(BUILD), '*.hip')))
    objects = [os.path.join(BUILD, os.path.basename(s)[:-4] + '.o') for s in sources]
    if not all(os.path.exists(f) for f in objects + TOOLS):
        pytest.skip('needs the objects of omg-tools_amd/csrc/build and the LLVM tools of ROCm')
    tmp = str(tmp_path_factory.mktemp('units'))
    return {os.path.basename(o)[:-2]: _kernels_of(o, tmp) for o in objects}


def test_every_kernel_is_compiled_in_exactly_one_unit(units):
    where = {}
    for unit, names in units.items():
        for n in names:
            where.setdefault(n, []).append(unit)
    twice = {n: u for n, u in where.items() if len(u) != 1}
    assert not twice, twice


def test_the_host_unit_holds_no_ipm_kernel_instance(units):
    assert 'omgx' in units and units['omgx'], sorted(units)
    assert [n for n in units['omgx'] if n.startswith(IPM)] == []


def test_the_kernels_are_the_committed_set(units):
    golden = open(os.path.join(ROOT, 'tests', 'golden', 'kernel_names.txt')).read().splitlines()
    assert sorted(n for names in units.values() for n in names) == golden
