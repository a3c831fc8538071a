# TEST-ONLY host build of the dedisperser's shared core, rtl-power-fftw_amd/csrc/dedisperse_core.h (the term, T, the tile
# partition, the span rule and the LDS index the kernel and the engine compile), with a CPU walk of the kernel's tiles:
# dedisperse_emul.cpp -> librpf_emul_dedisperse.so, loaded by tests/test_dedisperse.py and tests/test_gpu_dedisperse.py.
# A makefile of its own (make -f dedisperse.mk), as correlate.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_dedisperse.so: dedisperse_emul.cpp $(CSRC)/dedisperse_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ dedisperse_emul.cpp
clean:
	rm -f librpf_emul_dedisperse.so
.PHONY: clean
