# TEST-ONLY host build of the excised average over rtl-power-fftw_amd/csrc/excise_core.h (the element step the kernels
# compile, walked in their piece and group order): excise_emul.cpp -> librpf_emul_excise.so, loaded by
# tests/test_excise.py.  A makefile of its own (make -f excise.mk), as series_stats.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_excise.so: excise_emul.cpp $(CSRC)/excise_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ excise_emul.cpp
clean:
	rm -f librpf_emul_excise.so
.PHONY: clean
