// Host print-out of csrc/skip_rule.h, the rule that says which matrices of a transform's batch are dead and whose slots a pair's
// consumers read: a stand-alone program (its own main; build it with any host sanitizer).  One line per mode,
//   mode <number> one_content <0|1> one_style <0|1> dead <64 characters: matrix 0 .. 63, 1 = dead>
// which tests/test_skip_rule_cpu.py compares with a table of its own.  The predicates are called as the kernels call them, with
// the mode as an int.
#include "../../wct_tf_amd/csrc/skip_rule.h"

#include <cstdio>

int main() {
  const WctSkip modes[] = {WCT_SKIP_NONE, WCT_SKIP_SHARED_STYLE, WCT_SKIP_MIX, WCT_SKIP_STYLE, WCT_SKIP_CONTENT, WCT_SKIP_MIX_STYLE,
                           WCT_SKIP_STYLES};
  for (const WctSkip mode : modes) {
    const int skip = mode;
    printf("mode %d one_content %d one_style %d dead ", skip, one_content(skip) ? 1 : 0, one_style(skip) ? 1 : 0);
    for (int mat = 0; mat < 64; ++mat) putchar(skip_style_mat(mat, skip) ? '1' : '0');
    putchar('\n');
  }
  return 0;
}
