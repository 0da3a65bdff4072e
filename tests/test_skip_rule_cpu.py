"""csrc/skip_rule.h without a GPU: the skip mode of a transform's batch -- which of its matrices (matrix m = 2 * pair + side, side 0
the content, 1 the style) no stage computes, and whether a pair's consumers read pair 0's content or style slot -- printed by a
stand-alone host program and compared with a table written out here, mode by mode, from the sentences that define the modes."""
import os
import subprocess

import pytest

from conftest import ROOT

CLANG = '/opt/rocm/lib/llvm/bin/clang++'

# mode number: (name, is matrix m dead?, the shared slot: 'content' / 'style' of pair 0 for all pairs, or None)
RULE = {
    0: ('NONE', lambda m: False, None),                              # nothing is dead, no shared slot
    1: ('SHARED_STYLE', lambda m: m % 2 == 1 and m > 1, 'style'),    # the odd indices above 1; the style of pair 0 for all
    2: ('MIX', lambda m: m % 2 == 0 and m > 0, 'content'),           # the even indices above 0; the content of pair 0 for all
    3: ('STYLE', lambda m: m % 2 == 1, 'style'),                     # every odd index; the style of pair 0 for all
    4: ('CONTENT', lambda m: m % 2 == 0, None),                      # every even index; no shared slot
    5: ('MIX_STYLE', lambda m: m > 0, 'content'),                    # every index above 0; the content of pair 0 for all
    6: ('STYLES', lambda m: m % 2 == 1, None),                       # every odd index; no shared slot
}


@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_skip_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """Every mode, every matrix index 0 .. 63: dead or live, and per mode one_content / one_style, as the header computes them
    on the host.  A stand-alone program: nothing sanitized is loaded into this process."""
    exe = str(tmp_path / 'skip_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'skip_rule_check.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(RULE), out.stdout
    for mode, line in enumerate(lines):
        name, dead, shared = RULE[mode]
        expect = 'mode %d one_content %d one_style %d dead %s' % (
            mode, shared == 'content', shared == 'style', ''.join('1' if dead(m) else '0' for m in range(64)))
        assert line == expect, 'WCT_SKIP_%s' % name


def test_skip_modes_keep_their_numbers():
    """The enum of the header names all seven values with the numbers the kernels' argument words have always carried."""
    text = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'skip_rule.h')).read()
    body = text[text.index('enum WctSkip : int {'):]
    body = body[:body.index('};')]
    for mode, (name, _, _) in RULE.items():
        assert 'WCT_SKIP_%s = %d' % (name, mode) in body, name
    assert body.count('WCT_SKIP_') == len(RULE)
