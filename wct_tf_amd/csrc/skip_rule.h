// Which matrices of a transform's batch are dead, and whose slots their consumers read: the rule shared by the kernels and
// launchers of the whiten-colour transform and by any host program (plain C++: nothing of HIP is needed to include this file;
// tests/test_skip_rule_cpu.py pins the whole table).  The matrices of a batch of P pairs: matrix m = 2 * pair + side (0 content,
// 1 style).  No stage computes a dead matrix, and a consumer that would read it reads a live one, or a slot filled from a state:
//   mode           dead matrices            a pair's consumers read
//   NONE           none                     their own content and style slots
//   SHARED_STYLE   the odd m > 1            the style of pair 0          (one_style)
//   MIX            the even m > 0           the content of pair 0        (one_content)
//   STYLE          every odd m              the style of pair 0          (one_style)
//   CONTENT        every even m             their own slots
//   MIX_STYLE      every m > 0              the content of pair 0        (one_content)
//   STYLES         every odd m              their own slots
// SHARED_STYLE: one style image for every pair of the batch (video; WCT_FLAG_STYLE_SHARED) -- only pair 0's style matrix is
// computed.  MIX (launch_wct_mix) is the mirror image: K styles share ONE content, matrix 0.
// Prepared styles (wct_style, api.h): the style side of a call comes out of a handle's cached state, copied into the style slots
// by style_load_kernel (wct.hip), so EVERY style matrix is dead -- STYLE (P contents, one state in slot 1, read like a shared
// style) and MIX_STYLE (a mix of K states: matrix 0 alone is live).  CONTENT is the mirror image that fills a state: one style in
// slot 1, the content slot dead, no whitening side.  STYLES is the batched masked transform on prepared styles (mask.hip): every
// style matrix dead as under STYLE, but each pair reads the state in its OWN style slot.
#pragma once

#if defined(__HIPCC__)
#define WCT_SKIP_HD __device__ __host__ __forceinline__
#else
#define WCT_SKIP_HD inline
#endif

enum WctSkip : int {
  WCT_SKIP_NONE = 0, WCT_SKIP_SHARED_STYLE = 1, WCT_SKIP_MIX = 2, WCT_SKIP_STYLE = 3, WCT_SKIP_CONTENT = 4, WCT_SKIP_MIX_STYLE = 5,
  WCT_SKIP_STYLES = 6
};

// is matrix `mat` dead?  (an int: a kernel takes the mode as a plain argument or struct word.  The expression keeps the shape
// it has always had: hipcc's output for the ten kernels that inline it follows it.)
WCT_SKIP_HD bool skip_style_mat(int mat, int skip) {
  if (skip >= WCT_SKIP_STYLE)
    return skip == WCT_SKIP_STYLE ? (mat & 1) != 0
                                  : (skip == WCT_SKIP_CONTENT ? (mat & 1) == 0
                                                              : (skip == WCT_SKIP_MIX_STYLE ? mat > 0 : (mat & 1) != 0));
  return skip == WCT_SKIP_MIX ? ((mat & 1) == 0 && mat > 0) : (skip && (mat & 1) && mat > 1);
}
// which pair's slots hold the content / style moments a pair's consumers read: pair 0's for all where one is shared
WCT_SKIP_HD bool one_content(int skip) { return skip == WCT_SKIP_MIX || skip == WCT_SKIP_MIX_STYLE; }
WCT_SKIP_HD bool one_style(int skip) { return skip == WCT_SKIP_SHARED_STYLE || skip == WCT_SKIP_STYLE; }
