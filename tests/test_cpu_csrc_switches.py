"""The shipped HIP / C++ sources hold no compile-time switches (no GPU): every macro a conditional directive of
nerfactor_amd/csrc/ or include/nfx.h names is one of the few that are real — a source that builds two shipped translation
units, the header's include guard, the language / compiler checks.  Experiments live in git history (or as standalone
scripts/ubench/*.hip), not as a second kernel that a stray -D silently selects."""
import glob
import os
import re

from tests.conftest import ROOT

ALLOWED = {
    'NFX_GENERIC_TU',   # mlp_generic.hip included by mlp_generic_{x3,native}.hip
    'NFX_H_',           # include guard of include/nfx.h
    '__cplusplus',
    '__GNUC__',
}

_DIRECTIVE = re.compile(r'^\s*#\s*(ifdef|ifndef|if|elif)\b(.*)$')


def _sources():
    return sorted(glob.glob(os.path.join(ROOT, 'nerfactor_amd', 'csrc', '*'))) + [os.path.join(ROOT, 'include', 'nfx.h')]


def switches(paths):
    """(path, line number, macro) of every macro named by an #if / #ifdef / #ifndef / #elif directive."""
    found = []
    for path in paths:
        lines = open(path).read().split('\n')
        for no, line in enumerate(lines, 1):
            m = _DIRECTIVE.match(line)
            if not m:
                continue
            expr, k = m.group(2), no
            while expr.endswith('\\') and k < len(lines):
                expr = expr[:-1] + ' ' + lines[k]
                k += 1
            expr = re.sub(r'/\*.*?\*/', ' ', expr).split('//')[0]
            for name in re.findall(r'\b[A-Za-z_]\w*', expr):
                if name != 'defined':
                    found.append((path, no, name))
    return found


def test_sources_name_only_the_real_switches():
    bad = ['%s:%d: %s' % (os.path.relpath(p, ROOT), no, name) for p, no, name in switches(_sources()) if name not in ALLOWED]
    assert not bad, 'compile-time switches in the shipped sources:\n' + '\n'.join(bad)


def test_the_scan_reports_a_switch(tmp_path):
    src = tmp_path / 'k.hip'
    src.write_text('#include "x.hpp"\n#ifdef NFX_XP_FOO\n#endif\n#if defined(A) && B > 1  // C\n#endif\n')
    assert [(no, name) for _, no, name in switches([str(src)])] == [(2, 'NFX_XP_FOO'), (4, 'A'), (4, 'B')]
