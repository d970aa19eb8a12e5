"""The reference's own C example (c/example.c: three alignments through the 54-function C API) against
include/block_aligner_hip.h + libblock_aligner_hip.so ("example.c becomes a smoke test of our C-ABI lib").
The example's source is not part of this repository; tests/golden/reference_example_c_calls.json records the block_* functions it calls
(what `nm -u` listed for it compiled unchanged against this header and linked against this library). Every one of them must still be
declared by the header and resolve against the library: a C file of this test takes the address of each, compiled with -Wall -Werror."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "block_aligner_amd", "lib")
CALLS = os.path.join(ROOT, "tests", "golden", "reference_example_c_calls.json")


def test_reference_example_compiles_and_links_unchanged(tmp_path):
    with open(CALLS) as f:
        fns = json.load(f)["functions"]
    # the three expected answers -- score 12 twice and the profile alignment's -- are checked on the GPU by tests/test_c_abi.py's C caller,
    # which runs the same calls (c/example.c:8-33,41-81,90-125)
    assert "block_align_aa" in fns and "block_align_aa_trace" in fns and "block_align_profile_aa" in fns, fns
    src = tmp_path / "example_calls.c"
    # (an array with external linkage: the compiler keeps it, and with it a reference to every function)
    src.write_text('#include "block_aligner_hip.h"\n#include <stdio.h>\n\nvoid (*const example_calls[])(void) = {\n'
                   + "".join(f"    (void (*)(void))&{f},\n" for f in fns)
                   + "};\n\nint main(void) {\n    printf(\"%zu\\n\", sizeof example_calls / sizeof example_calls[0]);\n    return 0;\n}\n")
    exe = str(tmp_path / "example_calls")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L", LIBDIR, "-lblock_aligner_hip", f"-Wl,-rpath,{LIBDIR}"])
    # every block_* symbol the example calls resolves against the library (the link above would have failed otherwise)
    syms = subprocess.check_output(["nm", "-u", exe], text=True)
    used = sorted({l.split()[-1].split("@")[0] for l in syms.splitlines() if "block_" in l})
    assert used == sorted(fns), used
