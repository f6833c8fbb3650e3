# TEST-ONLY: the host code of LightClientAttackEvidence (csrc/lca_free.h, csrc/lca_host.h) as a
# stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, for
# tests/test_lca_host.py:  make -f lca_host.mk OUT=<dir>   (OUT: where the program is written)
CXX ?= g++
CSRC := ../../tendermint-fork_amd/csrc
OUT ?= .

$(OUT)/lca_host: lca_host.cpp $(wildcard $(CSRC)/*.h)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) lca_host.cpp -o $@
