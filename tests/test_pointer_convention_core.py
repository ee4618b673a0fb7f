"""The host-side checks every entry point of libm6a_hip.so shares (m6anet_amd/csrc/m6a_ctx.h: csr_check, same_side, enter, HintScope)
without a GPU: tests/pointer_convention_core_main.cpp as a program of its own under ASan and UBSan."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "pointer_convention_core")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "m6anet_amd", "csrc"),
                    os.path.join(HERE, "pointer_convention_core_main.cpp"), "-o", exe], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr and len(lines) == 24 and all(l.startswith("ok ") for l in lines), (r.returncode, r.stdout, r.stderr[-3000:])
