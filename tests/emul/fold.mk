# TEST-ONLY host build of the fold's shared core, rtl-power-fftw_amd/csrc/fold_core.h (the bin rule, the segment rule, the
# wave partition, the LDS index and the scratch layout the kernel and the engine compile), with a CPU walk of the kernel's
# waves: fold_emul.cpp -> librpf_emul_fold.so, loaded by tests/test_fold.py and tests/test_gpu_fold.py.
# A makefile of its own (make -f fold.mk), as dedisperse.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_fold.so: fold_emul.cpp $(CSRC)/fold_core.h ../../include/rpf_engine.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ fold_emul.cpp
clean:
	rm -f librpf_emul_fold.so
.PHONY: clean
