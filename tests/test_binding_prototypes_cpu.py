"""The ctypes prototypes of the binding are one table (`omgtools.backend.PROTOTYPES`), applied once by `load_library`: held here
against the declarations of include/omgx.h -- every declared entry the library exports has `argtypes`, as many as the declaration
has parameters."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ARGUMENTS = {'omgx_version', 'omgx_last_error'}


def _declarations():
    """name -> parameter count of every function the header declares."""
    text = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    mentioned = set(re.findall(r'\b(omgx_\w+)\s*\(', text))
    decl = {}
    for name, params in re.findall(r'\b(omgx_\w+)\s*\(([^()]*)\)\s*;', text):
        params = params.strip()
        decl[name] = 0 if params in ('', 'void') else params.count(',') + 1
    assert set(decl) == mentioned, 'declarations the pattern does not parse: %s' % sorted(mentioned - set(decl))
    return decl


def test_every_declared_entry_has_its_prototype_after_load_library():
    import ctypes
    from omgtools import backend as be
    decl = _declarations()
    assert len(decl) > 50 and decl['omgx_batch_solve'] == 10 and decl['omgx_version'] == 0
    lib = be.load_library()
    fresh = ctypes.CDLL(be.LIB_PATH)                   # (its own function objects: what it exports, no prototypes)
    for name, n_par in sorted(decl.items()):
        assert hasattr(fresh, name), name
        if name in NO_ARGUMENTS:
            continue
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name + ' has no argtypes'
        assert len(fn.argtypes) == n_par, (name, len(fn.argtypes), n_par)
        assert len(be.PROTOTYPES[name][1]) == n_par, name


def test_no_method_assigns_a_prototype():
    """`load_library` is the only place: no `.argtypes` / `.restype` assignment anywhere else in the package."""
    pkg = os.path.join(ROOT, 'omg-tools_amd', 'omgtools')
    hits = []
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith('.py'):
            for no, line in enumerate(open(os.path.join(pkg, fn)), 1):
                if re.search(r'\.(argtypes|restype)\b[^=]*=[^=]', line):
                    hits.append('%s:%d' % (fn, no))
    assert len(hits) == 1 and hits[0].startswith('backend.py:'), hits
