"""The wide-address instantiation of the model rounds' kernel body (model_group_rows<..., kWide = true> of
rsem_amd/csrc/model_block.hpp: window addresses of 40 bits, for references whose two strands take 4 GiB and more) against the
narrow one, run on the CPU by tests/model_wide_emu.cpp (one OS thread per lane, tests/simt_emu.hpp): a dozen transcripts, ~200
reads, reads of several 16-alignment chunks and runs of equal windows; the wide run sees the strands behind a pad that puts 2^32
(a) between two transcripts, (b) inside a forward strand with windows starting in the 8 bytes below it, (c) between a transcript's
two strands.  The pad is address space reserved with mmap(MAP_NORESERVE), never touched.  Without the update the kernel has no
atomics: conprb and noise conprb must be bit-identical.  Also the host's decision (window_addr_bits): which path for which
strand_bytes / pad, and the refusal above 2^40.  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(CC), reason="needs hipcc (host compilation of the HIP headers)")


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("model_wide_emu")), "model_wide_emu")
    r = subprocess.run([CC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value"] + os.environ.get("RSEM_EMU_FLAGS", "").split() + [
                        os.path.join(ROOT, "tests", "model_wide_emu.cpp"), "-o", exe, "-lpthread"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("model_type,seed", [(0, 11), (1, 12), (2, 13), (3, 14)])
def test_wide_addresses_give_the_bits_of_the_narrow_path(emulator, model_type, seed):
    r = subprocess.run([emulator, str(model_type), str(seed)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "MISMATCH" not in r.stdout
    assert r.stdout.count("bit-identical") == 3 and all("placement (%s)" % p in r.stdout for p in "abc")


def test_which_path_for_which_size(emulator):
    r = subprocess.run([emulator, "decide"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-3000:]
    # (the decisive rows, read back: what was accepted before stays narrow, what was refused is wide, 2^40 and more is refused)
    assert "strand_bytes 4294967272 pad 0 -> 32 bits" in r.stdout and "strand_bytes 4294967280 pad 0 -> 40 bits" in r.stdout
    assert "strand_bytes 1099511627760 pad 0 -> 0 bits" in r.stdout
