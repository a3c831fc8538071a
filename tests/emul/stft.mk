# TEST-ONLY host build of the short-time Fourier transform's plain-C++ parts over rtl-power-fftw_amd/csrc/stft_core.h
# (the staging index map the store kernels compile), k1_sizes.h and series_pieces.h (rpf_stft's piece rule):
# stft_emul.cpp -> librpf_emul_stft.so, loaded by tests/test_stft.py.  A makefile of its own (make -f stft.mk), as cross.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_stft.so: stft_emul.cpp $(CSRC)/stft_core.h $(CSRC)/fft_core.h $(CSRC)/k1_sizes.h $(CSRC)/rpf_device_common.h $(CSRC)/series_pieces.h
	$(CXX) -x hip --offload-host-only --rocm-path=/opt/rocm -O1 -std=c++17 -fPIC -ffp-contract=off -c -o stft_emul.host.o stft_emul.cpp
	$(CXX) -shared -o $@ stft_emul.host.o
	rm -f stft_emul.host.o
clean:
	rm -f librpf_emul_stft.so
.PHONY: clean
