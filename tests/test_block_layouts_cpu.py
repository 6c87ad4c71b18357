"""CPU: the output blocks are described twice -- the SAE_<BLOCK>_<FIELD> offset macros of include/freud_sae.h, which the engine
writes by, and the *_layout functions of freud_amd/engine.py, which every reader unpacks by.  A host C program prints every offset
and _BYTES of the five blocks; they must equal the Python layouts."""
import os
import subprocess

import pytest

from freud_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(0, 1, 96, 300), (3, 17, 256, 512), (8, 128, 1280, 24576)]           # (n_tau, K, d, n)
BLOCKS = {"STATS": (E.stats_layout, "n"), "RECON": (E.recon_layout, "n, d"), "FRONTIER": (E.frontier_layout, "n_tau, K, d"),
          "PURSUIT": (E.pursuit_layout, "n_tau, K, d, n"), "REFIT": (E.refit_layout, "n_tau, K, d, n")}


def layout(block, n_tau, K, d, n):
    fn, args = BLOCKS[block]
    return fn(*(dict(n_tau=n_tau, K=K, d=d, n=n)[a] for a in args.split(", ")))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """argv: n_tau K d n -> one line "BLOCK FIELD offset" per macro, in the order of the Python layouts."""
    lines = [f'  printf("{b} {f} %lld\\n", (long long)SAE_{b}_{f.upper()}({args}));' for b, (_fn, args) in BLOCKS.items()
             for f in layout(b, 0, 1, 1, 1)]
    src = ('#include <stdio.h>\n#include <stdlib.h>\n#include "freud_sae.h"\nint main(int argc, char** argv) {\n  if (argc != 5) return 2;\n'
           "  const long long n_tau = atoll(argv[1]), K = atoll(argv[2]), d = atoll(argv[3]), n = atoll(argv[4]);\n"
           "  (void)n_tau; (void)K; (void)d; (void)n;\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    tmp = tmp_path_factory.mktemp("layouts")
    path, exe = os.path.join(str(tmp), "layouts.c"), os.path.join(str(tmp), "layouts")
    with open(path, "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", f"-I{ROOT}/include", path, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_header_offsets_equal_the_python_layouts(prog, shape):
    out = subprocess.run([prog, *map(str, shape)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = [(b, f, int(v)) for b, f, v in (line.split() for line in out if line)]
    want = [(b, f, at if f == "bytes" else at[0]) for b in BLOCKS for f, at in layout(b, *shape).items()]
    assert got == want

