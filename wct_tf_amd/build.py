"""Build libwct_hip.so (gfx950) in-tree with hipcc.  `python -m wct_tf_amd.build`."""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libwct_hip.so')
# the whiten-colour transform is one unit per stage (csrc/wct_stages.h is what they share)
WCT_UNITS = ['stats_gemm.hip', 'eigh.hip', 'spectral.hip', 'wct.hip', 'mask.hip', 'style_swap.hip', 'warm.hip']
# the C ABI and its host-side orchestration, one unit per concern (csrc/api.h is what they share)
API_UNITS = ['api_ctx.hip', 'api_weights.hip', 'api_drivers.hip', 'api_ops.hip', 'api_stylize.hip', 'api_train.hip']
SOURCES = API_UNITS + ['conv.hip', 'conv_wino.hip', 'coral.hip', 'colors.hip', 'guided.hip', 'guided_color.hip', 'guided_time.hip', 'guided_motion.hip', 'guided_color_time.hip', 'guided_up.hip', 'guided_up_color.hip', 'guided_up_time.hip', 'noise.hip', 'resize.hip', 'banded.hip', 'wrap.hip', 'train.hip'] + WCT_UNITS


STAMP = LIB + '.src.sha256'
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-value', '-Wno-unused-result']
# per-file additions.  eigh.hip (with its jacobi_*.h): the SLP vectoriser packs the eigensolver's rotation arithmetic into v_pk_fma_f32 pairs at the
# price of ~20 v_mov per rotation set for operand assembly (measured: Jacobi 25.2 -> 23.8 ms per 32-pair step without it).  Only
# the eigensolver is known to need the flag; the other transform units carry it because they were built with it while they were
# one file with the solver, and nobody has measured them without it.
FILE_FLAGS = {u: ['-fno-slp-vectorize'] for u in WCT_UNITS}


def source_digest():
    """sha256 over every source the library is built from (csrc/*.hip, *.h, the public header) and the flags."""
    h = hashlib.sha256((' '.join(FLAGS) + repr(sorted(FILE_FLAGS.items()))).encode())
    deps = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.hip', '.h')))
    deps.append(os.path.join(os.path.dirname(HERE), 'include', 'wct_hip.h'))
    for d in deps:
        h.update(os.path.basename(d).encode())
        h.update(open(d, 'rb').read())
    return h.hexdigest()


def needs_build():
    """The .so is current iff the digest stored beside it equals the digest of the sources as they are now
    (modification times do not survive a snapshot to the GPU box; content does)."""
    if not (os.path.exists(LIB) and os.path.exists(STAMP)):
        return True
    return open(STAMP).read().strip() != source_digest()


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objs = [os.path.join(CSRC, src.replace('.hip', '.o')) for src in SOURCES]

    def compile_unit(src, obj):
        cmd = [hipcc] + FLAGS + FILE_FLAGS.get(src, []) + ['-c', os.path.join(CSRC, src), '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(min(16, len(SOURCES))) as pool:     # (a fixed bound, never the CPU count of the machine)
        list(pool.map(compile_unit, SOURCES, objs))
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(STAMP, 'w') as f:
        f.write(source_digest() + '\n')
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    print(LIB)
