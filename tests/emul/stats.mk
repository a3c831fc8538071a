# TEST-ONLY host build of K1's per-bin statistics (RPF_FLAG_BIN_STATS): the frame loop with phase_accumulate_stats and
# the slot / partial combine of fft_core.h, thread by thread: stats_emul.cpp -> librpf_emul_stats.so, loaded by
# tests/test_spectral_stats.py.  A makefile of its own (make -f stats.mk) beside the emulator's, as formats.mk;
# ROCm's clang because fft_core.h uses clang's ext_vector_type.
CXX := /opt/rocm/lib/llvm/bin/clang++
librpf_emul_stats.so: stats_emul.cpp ../../rtl-power-fftw_amd/csrc/fft_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ stats_emul.cpp
clean:
	rm -f librpf_emul_stats.so
.PHONY: clean
