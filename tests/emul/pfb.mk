# TEST-ONLY host build of the polyphase fold over rtl-power-fftw_amd/csrc/pfb_core.h (the conversion and the inner
# expression the kernels compile): pfb_emul.cpp -> librpf_emul_pfb.so, loaded by tests/test_pfb.py and
# tests/test_gpu_pfb.py.  A makefile of its own (make -f pfb.mk), as excise.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_pfb.so: pfb_emul.cpp $(CSRC)/pfb_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ pfb_emul.cpp
clean:
	rm -f librpf_emul_pfb.so
.PHONY: clean
