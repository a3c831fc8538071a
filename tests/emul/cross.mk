# TEST-ONLY host build of the cross-spectrum front end over rtl-power-fftw_amd/csrc/cross_core.h (the combined streams
# and the finishing expression the kernels compile): cross_emul.cpp -> librpf_emul_cross.so, loaded by
# tests/test_cross.py and tests/test_gpu_cross.py.  A makefile of its own (make -f cross.mk), as pfb.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_cross.so: cross_emul.cpp $(CSRC)/cross_core.h $(CSRC)/pfb_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ cross_emul.cpp
clean:
	rm -f librpf_emul_cross.so
.PHONY: clean
