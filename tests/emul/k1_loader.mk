# TEST-ONLY host build of the schedule of K1's loader waves (rtl-power-fftw_amd/csrc/k1_loader.h, plain C++):
# k1_loader_emul.cpp -> librpf_emul_k1_loader.so, loaded by tests/test_k1_loader_schedule.py.  A makefile of its own
# (make -f k1_loader.mk), as stft.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_k1_loader.so: k1_loader_emul.cpp $(CSRC)/k1_loader.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -o $@ k1_loader_emul.cpp
clean:
	rm -f librpf_emul_k1_loader.so
.PHONY: clean
