"""The queue and the lane loop of zk_pipeline (csrc/pipeline_lanes.h) under ThreadSanitizer, without a GPU: a stand-alone
program over fake lanes (tests/pipeline_lanes_main.cpp), built with the clang of the emulation build and run as a child."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CLANGXX = os.path.join(ROCM, "lib", "llvm", "bin", "clang++")


def test_pipeline_lanes_under_thread_sanitizer(tmp_path):
    cxx = CLANGXX if os.path.exists(CLANGXX) else "clang++"
    exe = str(tmp_path / "pipeline_lanes")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", os.path.join(HERE, "pipeline_lanes_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0 and "ThreadSanitizer" not in run.stderr, run.stdout + run.stderr
    assert "all scenarios held" in run.stdout
