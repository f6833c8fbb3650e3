# TEST-ONLY: host (CPU) build of the half-size path's joint radix-4 table (joint_host.cpp) for
# tests/test_joint_table_host.py and tests/test_gpu_joint_table.py:  make -f joint_host.mk
CXX ?= g++
CSRC := ../../tendermint-fork_amd/csrc

libjointhost.so: joint_host.cpp $(wildcard $(CSRC)/*.h)
	$(CXX) -O2 -fPIC -shared -std=c++17 -I$(CSRC) joint_host.cpp -o $@
