"""K23's packer (corda_amd/csrc/sig_pack.hpp) on the host under AddressSanitizer + UBSan:
tools/sig_pack_check.cpp replays the count, scan and pack passes tile by tile, the wave
ballots emulated, with the header's own functions into buffers of exactly the sizes the layout
names, and compares every row, pre-status, lane_of_row, message index, perm, count and header
word with a plain sequential run of the host packer (pack_rows.hpp) over the same batch; the
lane rule is checked against a restatement of it as well. A stand-alone program: nothing is
loaded into Python."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_sig_pack_passes_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sig_pack_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "sig_pack_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20261021"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["failures"] == 0, st
    # overlapping key ranges (more lanes of an RSA class than key_bytes holds keys for): the lanes past
    # the class's rows are bad-range lanes, the counts are clipped; with disjoint ranges it never happens
    assert st["overlap_cases"] == 6 and st["over_cap"] > 1000, st
    # 9 lane counts x (the mix, each of the 7 classes alone, each of them absent) x (in order, shuffled),
    # 3 lane counts x 3 places x 5 kinds of bad range, 16 source misalignments
    assert st["cases"] == 9 * 15 * 2 + 3 * 3 * 5 + 6 + 16 and st["shuffled"] >= 9 * 15, st
    assert st["n0"] == 30 and st["multi_tile"] >= 30 and st["rule_checks"] > 100000, st
    # every class met, empty in some case and owning every lane in another
    assert all(c > 1000 for c in st["class_lanes"]), st
    assert all(c >= 16 for c in st["empty_class_cases"]) and all(c >= 16 for c in st["single_class_cases"]), st
    # key lengths 0/31/32/33/64/65/66; ECDSA signature lengths 0/8/72/73/80, over-long both ways
    assert all(c > 100 for c in st["key_len_seen"]) and all(c > 100 for c in st["ec_sig_len_seen"]), st
    assert st["ec_long_wellformed"] > 100 and st["ec_long_garbage"] > 100, st
    # RSA: every width class, every corner of the key rule once by construction, the over-long signature
    assert all(c > 1000 for c in st["rsa_class_rows"]) and st["rsa_sig_long"] > 100, st
    for k in ("rsa_even_n", "rsa_e_even", "rsa_e_lt3", "rsa_e_big", "rsa_1016", "rsa_4104", "rsa_trunc"):
        assert st[k] == 1, (k, st)
    assert st["rsa_flag_off_lanes"] > 100, st
    # the direct statuses the rule gives: BAD_SIG, BAD_KEY, UNSUPPORTED, EMPTY
    assert all(st["direct_status"][s] > 100 for s in (1, 3, 4, 5)), st
    # reversed and overrunning ranges and a message row out of bounds, in the first, a middle and the last lane
    assert st["bad_first"] == st["bad_mid"] == st["bad_last"] == 15, st
    assert st["bad_reversed"] == 18 and st["bad_overrun"] == 18 and st["bad_msg_row"] == 9, st
    # every source misalignment 0..15, keys and signatures
    assert all(c > 100 for c in st["key_align"]) and all(c > 100 for c in st["sig_align"]), st


def test_bad_range_status_matches_header_and_packer():
    """CORDAHIP_STATUS_BAD_RANGE is defined with parentheses (the plain-numbered CORDAHIP_STATUS_* are
    Crypto.kt's six): the header, the Python binding and the packer's constant agree, and 19 is used by
    no other per-lane status of the signature calls."""
    import re
    import sys
    sys.path.insert(0, ROOT)
    from corda_amd import _lib
    src = open(os.path.join(ROOT, "include", "cordahip.h")).read()
    m = re.findall(r"#define CORDAHIP_STATUS_BAD_RANGE \((\d+)\)", src)
    assert m == ["19"] and _lib.BAD_RANGE == 19
    hpp = open(os.path.join(ROOT, "corda_amd", "csrc", "sig_pack.hpp")).read()
    assert re.search(r"kStBadRange = 19\b", hpp)
    taken = {int(v) for v in re.findall(r"#define CORDAHIP_(?:STATUS|SIGN|VERIFY|TX|COMMIT)_\w+ \(?(\d+)\)?", src)}
    assert taken >= {0, 1, 2, 3, 4, 5, 19} and max(taken) == 19
