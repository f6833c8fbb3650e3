# TEST-ONLY: the host replay of validateBlock (csrc/validate_host.h) as a stand-alone program under
# AddressSanitizer and UndefinedBehaviorSanitizer, for tests/test_validate_host.py:
#   make -f validate_host.mk OUT=<dir>   (OUT: where the program is written)
CXX ?= g++
CSRC := ../../tendermint-fork_amd/csrc
OUT ?= .

$(OUT)/validate_host: validate_host.cpp $(wildcard $(CSRC)/*.h)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) validate_host.cpp -o $@
