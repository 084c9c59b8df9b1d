"""The table cache of the host layer (omg-tools_amd/csrc/omgx_table_cache.h) on a CPU: a stand-alone C++ program drives it with a
fake allocator, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ['same_content_same_entry', 'one_byte_new_entry', 'other_size_new_entry', 'other_device_new_entry',
         'last_release_frees_once', 'take_after_free_rebuilds', 'failures_leave_nothing', 'threads_end_with_nothing_live']


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('table_cache') / 'table_cache')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', os.path.join(ROOT, 'tests', 'cpp', 'table_cache.cpp'), '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return run.returncode, run.stdout.decode(), run.stderr.decode()


def test_program_runs_clean_under_the_sanitizers(report):
    rc, out, err = report
    assert rc == 0 and 'ERROR' not in err and 'runtime error' not in err, (rc, out, err)


@pytest.mark.parametrize('case', CASES)
def test_case(report, case):
    rc, out, err = report
    assert 'ok ' + case in out.split('\n'), (case, out, err)
