"""The host code of the library stands on the data layout of the solve alone (omg-tools_amd/csrc/omgx_types.h), the wave path's
linear solve reads on its own (omgx_kkt_wave.h, device only), and the entry points of the linear solve in omgx_core.h hold no code
of the other target.  Checked on the text and with the host compiler, without a device:
  * omgx_types.h and omgx_core.h compile on their own as the host twin sees them (self-contained headers);
  * the host unit, the plan and the shared kernel-argument header include no solver header but omgx_types.h, so an edit to the
    factorisation or the iteration does not rebuild them;
  * no target #ifdef between the braces of the five entry points of the linear solve."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'omg-tools_amd', 'csrc')
DEVICE_ONLY = ('omgx_kkt_wave.h', 'omgx_wave.h')      # gfx950 intrinsics: no host twin
SOLVER_HEADERS = ('omgx_types.h', 'omgx_core.h') + DEVICE_ONLY
HOST_SIDE = ('omgx_plan.h', 'omgx.hip', 'omgx_device.h')
ENTRY_POINTS = ('kkt_factor', 'kkt_refactor_root', 'kkt_root_before_retry', 'kkt_solve', 'kkt_solve2')


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def _includes(text):
    return re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, flags=re.M)


@pytest.mark.parametrize('header', ['omgx_types.h', 'omgx_core.h'])
def test_header_is_self_contained_on_the_host(header, tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('needs g++')
    unit = tmp_path / 'alone.cpp'
    unit.write_text('#include "%s"\n' % header)
    r = subprocess.run([gxx, '-std=c++17', '-DOMGX_HOST_PORT', '-fsyntax-only', '-I', CSRC, str(unit)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]


def test_the_wave_path_reaches_device_builds_only():
    core = _text('omgx_core.h')
    assert _includes(core) == ['omgx_types.h', 'omgx_kkt_wave.h']
    assert re.search(r'^#ifndef OMGX_HOST_PORT\n#include "omgx_kkt_wave.h"[^\n]*\n#endif\n', core, flags=re.M)
    assert _includes(_text('omgx_kkt_wave.h')) == ['omgx_wave.h']


@pytest.mark.parametrize('name', HOST_SIDE)
def test_host_side_includes_the_types_header_and_no_other_solver_header(name):
    inc = [os.path.basename(i) for i in _includes(_text(name))]
    assert 'omgx_types.h' in inc, inc
    assert [i for i in inc if i in SOLVER_HEADERS and i != 'omgx_types.h'] == [], inc
    # and what they include of the library's own does not bring the solver back in
    for i in inc:
        if i.startswith('omgx_') and i not in SOLVER_HEADERS and os.path.exists(os.path.join(CSRC, i)):
            deeper = [os.path.basename(j) for j in _includes(_text(i))]
            assert [j for j in deeper if j in SOLVER_HEADERS and j != 'omgx_types.h'] == [], (i, deeper)


def test_the_types_header_names_no_context_and_no_intrinsic():
    code = re.sub(r'//[^\n]*', '', _text('omgx_types.h'))
    for word in ('Ctx', 'threadIdx', 'blockIdx', '__builtin_amdgcn', '__syncthreads', 'OMGX_PFOR'):
        assert word not in code, word
    assert _includes(_text('omgx_types.h')) == []


def _bodies(text, name):
    """text between the braces of every definition of the function template `name` (a signature that ends in ') {')"""
    out = []
    for m in re.finditer(r'^OMGX_FN \w+ %s\(const C& c,[^{;]*\) \{' % re.escape(name), text, flags=re.M):
        depth, i = 1, m.end()
        while depth:
            ch = text[i]
            depth += (ch == '{') - (ch == '}')
            i += 1
        out.append(text[m.end():i - 1])
    return out


def _target_sections(core):
    """(device section, host-twin section) of the linear solve in omgx_core.h: the two arms of the #ifndef OMGX_HOST_PORT that
    holds kkt_solve2_blocked"""
    start = core.rindex('#ifndef OMGX_HOST_PORT\n', 0, core.index('OMGX_FN void kkt_solve2_blocked('))
    mid = core.index('\n#else\n', start)
    end = core.index('\n#endif\n', core.index('OMGX_FN void kkt_solve2(', core.index('OMGX_FN void kkt_solve2_host(', mid)))
    return core[start + len('#ifndef OMGX_HOST_PORT\n'):mid], core[mid + len('\n#else\n'):end]


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_point_of_the_linear_solve_holds_no_target_ifdef(name):
    core = _text('omgx_core.h')
    device, host = _target_sections(core)
    # one definition per target, each inside the section of its target; no body is spliced from two targets
    assert len(_bodies(device, name)) == 1 and len(_bodies(host, name)) == 1 and len(_bodies(core, name)) == 2, name
    for body in _bodies(core, name):
        assert 'OMGX_HOST_PORT' not in body, body


def test_the_sections_of_the_linear_solve_hold_no_target_ifdef_at_all():
    for section in _target_sections(_text('omgx_core.h')):
        assert 'OMGX_HOST_PORT' not in section


@pytest.mark.parametrize('name', [n for n in ENTRY_POINTS if n != 'kkt_factor'])
def test_entry_point_is_a_selection_of_named_bodies(name):
    # (kkt_factor on the device holds the blocked factorisation itself: see its comment)
    for body in _bodies(_text('omgx_core.h'), name):
        assert len(body.strip().splitlines()) <= 2, body
    host = _target_sections(_text('omgx_core.h'))[1]
    assert len(_bodies(host, 'kkt_factor')[0].strip().splitlines()) == 1
