"""Every internal host function of libnfx.so is declared once (no GPU): nerfactor_amd/csrc/launchers.hpp holds the launchers,
their size / plan queries and the option lookup, capi_common.hpp the error helpers of the C-ABI files, and both the
definition and every caller include them — so a parameter list that drifts is a compile error, not arguments read from the
wrong registers.  No .hip or .cpp file writes a prototype of its own."""
import glob
import os
import re

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'nerfactor_amd', 'csrc')
DECLARING_HEADERS = ('launchers.hpp', 'capi_common.hpp')

# a declarator at the start of a line: [extern "C"] [attributes] return type, nfx_<name>, '('
_HEAD = re.compile(r'^[ \t]*(?:extern\s+"C"\s+)?(?:__attribute__\(\(.*?\)\)\s*)?(?:[A-Za-z_][\w:]*[ \t\*&]+)+(nfx_\w+)\s*\(', re.M)


def _blank(src):
    """src with comments, string and character literals blanked out (same length, same line breaks)."""
    def spaces(m):
        return re.sub(r'[^\n]', ' ', m.group(0))
    return re.sub(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', spaces, src, flags=re.S)


def prototypes(paths):
    """(path, line number, name) of every nfx_* function declared without a body: a declarator at the start of a line whose
    parameter list, possibly over several lines, is followed by ';'."""
    found = []
    for path in paths:
        src = _blank(open(path).read())
        for m in _HEAD.finditer(src):
            if re.match(r'\s*(return|else|case|goto|throw|new|delete)\b', m.group(0)):
                continue      # an expression statement such as `return nfx_f(...);`
            depth, k = 1, m.end()
            while depth and k < len(src):
                depth += {'(': 1, ')': -1}.get(src[k], 0)
                k += 1
            if re.match(r'\s*;', src[k:]):
                found.append((path, src.count('\n', 0, m.start(1)) + 1, m.group(1)))
    return found


def _units():
    return sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.cpp')))


def _count(needle):
    return sum(open(p).read().count(needle) for p in sorted(glob.glob(os.path.join(CSRC, '*'))))


def test_no_translation_unit_declares_an_internal_function():
    bad = ['%s:%d: %s' % (os.path.relpath(p, ROOT), no, name) for p, no, name in prototypes(_units())]
    assert not bad, 'prototypes outside %s:\n%s' % (' / '.join(DECLARING_HEADERS), '\n'.join(bad))


def test_the_headers_declare_and_every_c_abi_file_includes_them():
    declared = {name for _, _, name in prototypes([os.path.join(CSRC, h) for h in DECLARING_HEADERS])}
    assert {'nfx_option_int', 'nfx_fail', 'nfx_hip_result', 'nfx_launch_wgrad_batch_counted', 'nfx_generic_bwd_m2'} <= declared
    others = [p for p in glob.glob(os.path.join(CSRC, '*.hpp')) if os.path.basename(p) not in DECLARING_HEADERS]
    assert not prototypes(others)
    for path in glob.glob(os.path.join(CSRC, 'capi*.cpp')):
        assert '#include "capi_common.hpp"' in open(path).read(), path


def test_shared_definitions_exist_once():
    assert _count('struct nfx_wgrad_call {') == 1
    assert _count('#define REQUIRE') == 1
    assert _count('#define ALIGNED') == 1


def test_the_scan_reports_prototypes_and_not_definitions(tmp_path):
    src = tmp_path / 'k.hip'
    src.write_text('#include "x.hpp"\n'
                   'extern "C" int nfx_launch_one(const float*, long long, hipStream_t);   // one line\n'
                   'size_t nfx_two_bytes(const nfx::generic::Args* a,\n'
                   '                     int n);\n'
                   '// int nfx_in_a_comment(int);\n'
                   'int nfx_launch_three(const float* x, int n) {\n'
                   '    if (n <= 0) return nfx_fail(1, "int nfx_in_a_string(int);");\n'
                   '    return nfx_launch_one(x, n, 0);\n'
                   '}\n')
    assert [(no, name) for _, no, name in prototypes([str(src)])] == [(2, 'nfx_launch_one'), (3, 'nfx_two_bytes')]
