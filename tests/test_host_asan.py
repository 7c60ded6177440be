"""The host-side compiler (definition language -> regexps -> automata -> table blob -> hop tier tables -> the batch kernels' table
images and the kernel a batch gets; no HIP involved) built with AddressSanitizer + UndefinedBehaviorSanitizer and run over the golden
definitions and mutated copies of them.
(GPU AddressSanitizer is not available on the GPU pool: sanitizers run on the CPU build only.)"""
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorp_amd", "csrc")


def _golden_definitions():
    out = []

    def walk(o):
        if isinstance(o, dict):
            for k, v in o.items():
                if k == "def" and isinstance(v, str):
                    out.append(v)
                else:
                    walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)

    gdir = os.path.join(ROOT, "tests", "golden")
    for f in sorted(os.listdir(gdir)):
        if f.endswith(".json"):
            walk(json.load(open(os.path.join(gdir, f))))
    return out


def test_host_compiler_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "asan_driver")
    srcs = [os.path.join(ROOT, "tests", "cpp", "asan_driver.cpp")] + [os.path.join(CSRC, f) for f in
                                                                        ("gx_regex.cpp", "gx_compile.cpp", "gx_host.cpp", "gx_dsl.cpp", "gx_json.cpp", "gx_hop.cpp",
                                                                         "gx_images.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", CSRC, "-I",
           os.path.join(ROOT, "include")] + srcs + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    defs = _golden_definitions()
    assert len(defs) >= 8
    rng = random.Random(11)
    alphabet = "%@$(){}[]\\\"'#\n\t |*+?.,:=abc019"
    texts = list(defs)
    for _ in range(400):   # mutated copies: the parser's error paths
        t = list(rng.choice(defs))
        for _ in range(rng.randint(1, 6)):
            if not t:
                break
            op, pos = rng.random(), rng.randrange(len(t))
            if op < 0.4:
                del t[pos]
            elif op < 0.8:
                t.insert(pos, rng.choice(alphabet))
            else:
                t[pos] = rng.choice(alphabet)
        texts.append("".join(t))
    # one definition whose extraction is too ambiguous for an automaton built ahead of time (blank-separated fields that may be empty:
    # gx_compile.cpp keeps its program, blob version 3) -- packed, unpacked and damaged like the others
    texts.append("pattern %f \\S*\nextract fields {\n  template " + " ".join("$f%d(%%f)" % k for k in range(13)) + "\n}\n")
    paths = []
    for i, t in enumerate(texts):
        p = tmp_path / ("d%04d.grp" % i)
        p.write_text(t, encoding="utf-8")
        paths.append(str(p))
    # the README definition (gorp_amd/workloads.py: readme3_definition), whose kernel choice is pinned below
    readme = tmp_path / "readme.grp"
    readme.write_text("pattern %num \\d+\npattern %word \\w+\npattern %phrase \\S+\n" + "".join(
        "extract %s {\n  template [$timestamp(%%num)]: $verb(%s) $timeTakenInMsec(%%num)ms $path(%%phrase)\n}\n" % (name, verb)
        for name, verb in (("PutRequest", "PUT"), ("GetRequest", "GET"), ("OtherRequest", "%word"))), encoding="utf-8")
    paths += ["--pin", str(readme)]
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
    assert "asan driver: " in out
    compiled = int(out.split("asan driver: ")[1].split()[0])
    assert compiled >= len(defs) + 2   # every golden definition compiles, the one that is run as a program, and the README one
    # table images under seven sets of GX_CREATE_* flags, and plan_batch over 7 line lengths x 32 batch shapes x 7 kernels for each: every
    # plan uses images that exist, and its LDS layout fits
    assert int(out.split("batch plans: ")[1].split()[0]) >= compiled * 7 * 7 * 32 * 7
    # The kernel AUTO picks (GX_KERNEL_*; n: the UTF-16 units are narrowed to bytes first) for: captures with lines of 200 bytes, of
    # 200 uneven, of 400, of 1500; match only; match only with the states (gx_match_batch); UTF-16 units, lines of 200, of 1500;
    # GX_KERNEL_HOP_SLICES named; GX_KERNEL_PER_LINE named.  The same choice as the GPU tests see through gx_stat(h, 25).
    pins = dict(line.split(": ", 1) for line in out.splitlines() if line.startswith("pin " + str(readme)))
    # dense rows in LDS: the tile kernel, the slice kernel for long lines; no hop tables to take a UTF-16 batch's long lines
    assert pins["pin %s 0" % readme].split() == "1 1 1 2 1 1 1 n 1 3".split()
    # GX_CREATE_TIER_HOP: the tile kernel on hop tables, the hop slice kernel for long or uneven lines; the states only from dense rows
    assert pins["pin %s 64" % readme].split() == "5 6 6 6 5 1 5 6 6 3".split()
    # the hop tier's tables (gx_hop.cpp), walked on the host as the kernel walks them, agree with the dense automaton
    hop_defs, hop_lines = [int(x) for x in out.split("hop tier: ")[1].replace(" definitions,", "").split()[:2]]
    assert hop_defs >= len(defs) // 2 and hop_lines >= 400 * hop_defs
    # ... and some of those lines went through a loop set's second chance (\w fields hold digits and upper case)
    assert int(out.split("lines agree with the dense automaton (")[1].split()[0]) > 0
