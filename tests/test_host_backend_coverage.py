"""Keeps test_gpu_ops.py's docstring true: every public HipBackend method that issues a launch is called by some GPU
test (tests/test_gpu_*.py).  CPU-only: ops.py is parsed, not imported."""
import ast
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
OPS = os.path.join(os.path.dirname(HERE), "masters-thesis_amd", "ops.py")

# Pure query helpers: they read a size, a plan or a capability from the library (or build a descriptor on the host) and
# launch nothing, so no kernel test has to call them.
QUERY_HELPERS = {
    "bn_nchunk",                     # BatchNorm partial-chunk count
    "gemm_fused_cfg",                # configuration the one-round GEMM would pick
    "gemm3_plan",                    # (tile, split) of the gemm3 cost model
    "gemm3_work_floats",             # workspace sizes
    "gemm3_sync_words",
    "gemm3_pair_supported",          # capability queries
    "lstm_seq_supported",
    "gemm3_desc",                    # host-side descriptors
    "finalize_desc",
    "lstm_seq_bwd_work_floats",
    "lc_seq_fwd_work_floats",
    "lc_seq_bwd_work_floats",
    "attention_front_bwd_parts",     # partial counts
    "attention_metric_parts",
    "embedding_bwd_parts",
}


def _backend_methods():
    tree = ast.parse(open(OPS).read(), OPS)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "HipBackend")
    out = {}
    for fn in cls.body:
        if not isinstance(fn, ast.FunctionDef) or fn.name.startswith("_"):
            continue
        launches = any(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "_call"
                       for n in ast.walk(fn))
        out[fn.name] = launches
    return out


def test_every_launching_backend_method_has_a_gpu_test():
    methods = _backend_methods()
    assert len(methods) > 50, "HipBackend not found in ops.py"
    sources = "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py"))))
    missing = sorted(m for m, launches in methods.items()
                     if launches and not re.search(r"\." + re.escape(m) + r"\(", sources))
    assert not missing, f"HipBackend methods no tests/test_gpu_*.py calls: {missing}"


def test_query_helper_list_is_exact():
    """every public method either launches (through HipBackend._call) or is a listed query helper, and no listed helper
    launches: a new entry point cannot slip past the check above by not being recognised as a launch"""
    methods = _backend_methods()
    unlisted = sorted(m for m, launches in methods.items() if not launches and m not in QUERY_HELPERS)
    assert not unlisted, f"public HipBackend methods that launch nothing and are not listed as query helpers: {unlisted}"
    wrong = sorted(m for m in QUERY_HELPERS if methods.get(m, True))
    assert not wrong, f"listed as query helpers but missing or launching: {wrong}"
