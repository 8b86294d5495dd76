"""The bookkeeping of the BAL front end's partial-sum stage (ceres-solver_amd/csrc/partial_sums.h, design/25_partial_sums.md): the part
without HIP in it — capacity, position, room, take, drop, sets — compiled with g++ into a stand-alone program and run, once plainly and
once with the address and undefined-behaviour sanitizers (nothing is preloaded: the program has its own main).

Sets carry no generation.  A set is good from its take() to the first room() after the collect() or drop() that follows; holding one
longer is the caller's mistake, not something the ledger detects — the program states what a set taken after a drop looks like (the
same offsets again) rather than checking a stamp."""
import os
import subprocess
import textwrap

import pytest

from conftest import ROOT

CHECK = """
    #include <cstdio>
    #include "partial_sums.h"

    #define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\\n", __LINE__, #cond); return 1; } } while (0)

    int main() {
      chip::PartialLedger L;
      L.capacity = 8;
      // room(4), take(2), take(1): offsets 0 and 2, position 3 — packed, no gap for the doubles room() allowed and nobody took
      EXPECT(L.room(4) == 0);
      const chip::PartialSet a = L.take(2), b = L.take(1);
      EXPECT(a.offset == 0 && a.count == 2);
      EXPECT(b.offset == 2 && b.count == 1);
      EXPECT(L.position == 3 && L.error.empty());
      // 5 are free: 6 are refused with a message naming the request and what is free, and nothing moves
      EXPECT(L.room(6) == -1);
      EXPECT(L.position == 3);
      EXPECT(L.error.find("6") != std::string::npos && L.error.find("5 of 8 free") != std::string::npos);
      L.error.clear();
      EXPECT(L.room(5) == 3 && L.error.empty());
      // a take beyond what the last room() granted is refused: an empty set, the position stays
      EXPECT(L.take(2).count == 2 && L.position == 5);
      const chip::PartialSet over = L.take(4);   // 3 of the 5 granted are left
      EXPECT(over.count == 0 && L.position == 5 && !L.error.empty());
      L.error.clear();
      EXPECT(L.take(3).count == 3 && L.position == 8 && L.error.empty());
      // full: not one more
      EXPECT(L.room(1) == -1 && L.position == 8);
      L.error.clear();
      EXPECT(L.room(0) == 8 && L.take(0).count == 0 && L.error.empty());
      // a grant does not outlive the next room(): room(2) after room(5) allows 2
      L.drop();
      EXPECT(L.position == 0);
      EXPECT(L.room(8) == 0 && L.error.empty());
      EXPECT(L.room(2) == 0);
      EXPECT(L.take(3).count == 0 && L.position == 0 && !L.error.empty());
      L.error.clear();
      // after a drop the stage starts over: the first set lies where `a` lay.  No generation tells the two apart — a caller reads a
      // set before its next room(), that is the contract
      EXPECT(L.room(4) == 0);
      const chip::PartialSet c = L.take(2);
      EXPECT(c.offset == a.offset && c.count == a.count);
      L.drop();
      // no room was granted since the drop: nothing can be taken
      EXPECT(L.take(1).count == 0 && L.position == 0);
      // negative requests are refused
      L.error.clear();
      EXPECT(L.room(-1) == -1 && !L.error.empty());
      std::printf("partial sums ok\\n");
      return 0;
    }
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_partial_sum_ledger(tmp_path, flags):
    src = tmp_path / "partial_sums_check.cc"
    src.write_text(textwrap.dedent(CHECK))
    exe = tmp_path / "partial_sums_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + [
        "-I", os.path.join(ROOT, "ceres-solver_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "partial sums ok" in r.stdout, r.stdout + r.stderr
