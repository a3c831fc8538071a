# TEST-ONLY host build of the correlator's shared core, rtl-power-fftw_amd/csrc/correlate_core.h (the per-frame term, the
# pair -> plane map, the frame-group partition and the chunk rule the kernels and the engine compile):
# correlate_emul.cpp -> librpf_emul_correlate.so, loaded by tests/test_correlate.py and tests/test_gpu_correlate.py.
# A makefile of its own (make -f correlate.mk), as cross.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_correlate.so: correlate_emul.cpp $(CSRC)/correlate_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ correlate_emul.cpp
clean:
	rm -f librpf_emul_correlate.so
.PHONY: clean
