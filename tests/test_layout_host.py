"""The block layout builder and the tile envelope (csrc/plba_layout.hpp) and the problem table and plans
of the association calls (csrc/plba_assoc_plan.hpp) on the host: a stand-alone program
(tests/cpp/layout_check.cpp) built with the address and undefined-behaviour sanitizers, run as a child
process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
RUNNER = os.path.join(HERE, "cpp", "layout_check")


def test_layout_and_tile_envelope_host_program():
    assert os.path.exists(RUNNER), "build() makes tests/cpp/layout_check"
    r = subprocess.run([RUNNER], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "layout_check ok" and r.stderr == ""
