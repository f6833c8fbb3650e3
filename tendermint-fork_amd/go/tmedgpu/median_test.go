package tmedgpu

// MedianTimes against the three cases the reference pins (types/time/time_test.go:10-56) and the
// outcomes that need no median: nothing entering, and the inputs left to the Go path.
// Not run in this repository (no Go toolchain); tools/go_cgo_check.py type-checks it.

import (
	"testing"
)

const medianT1 = int64(1700000000)

// medianFixture: validator i has address {i+1, 0, ...} and power powers[i]; signature i is
// validator i's, sent offsets[i] seconds after medianT1, absent where offsets[i] < 0.
func medianFixture(offsets []int64, powers []int64) (*CommitData, *ValSet) {
	n := len(powers)
	vals := &ValSet{PubKeys: make([]byte, 32*n), Powers: powers, Addresses: make([]byte, 20*n)}
	cm := &CommitData{Flags: make([]byte, n), Addresses: make([]byte, 20*n), AddrLens: make([]uint32, n),
		TsSeconds: make([]int64, n), TsNanos: make([]int32, n), Sigs: make([]byte, 64*n), SigLens: make([]uint32, n)}
	for i := 0; i < n; i++ {
		vals.Addresses[20*i] = byte(i + 1)
		cm.Addresses[20*i] = byte(i + 1)
		cm.AddrLens[i] = 20
		cm.Flags[i] = 2
		if offsets[i] < 0 {
			cm.Flags[i] = 1
			continue
		}
		cm.TsSeconds[i] = medianT1 + offsets[i]
		cm.TsNanos[i] = 123456789
	}
	return cm, vals
}

func TestMedianTimesReferenceCases(t *testing.T) {
	e := engineOrSkip(t)
	reqs := make([]MedianRequest, 3)
	reqs[0].Commit, reqs[0].Vals = medianFixture([]int64{5, 10, 0}, []int64{40, 27, 33})
	reqs[1].Commit, reqs[1].Vals = medianFixture([]int64{10, 0, 5}, []int64{33, 40, 27})
	reqs[2].Commit, reqs[2].Vals = medianFixture([]int64{15, 5, -1, 0, 10, 5, -1, 60}, []int64{20, 10, 5, 10, 23, 10, 5, 10})
	want := []int64{5, 5, 10}
	entered := []uint32{3, 3, 6}
	res, err := e.MedianTimes(reqs)
	if err != nil {
		t.Fatal(err)
	}
	for i := range res {
		if res[i].Code != MedianOK || res[i].Seconds != medianT1+want[i] || res[i].Nanos != 123456789 {
			t.Fatalf("case %d: code %d time %d.%09d", i, res[i].Code, res[i].Seconds, res[i].Nanos)
		}
		if res[i].Entered != entered[i] || !res[i].OnDevice {
			t.Fatalf("case %d: entered %d on device %v", i, res[i].Entered, res[i].OnDevice)
		}
	}
}

func TestMedianTimesZeroTimeAndGoPath(t *testing.T) {
	e := engineOrSkip(t)
	reqs := make([]MedianRequest, 4)
	// every signature absent
	reqs[0].Commit, reqs[0].Vals = medianFixture([]int64{-1, -1}, []int64{1, 1})
	// a negative power
	reqs[1].Commit, reqs[1].Vals = medianFixture([]int64{0, 1}, []int64{1, -1})
	// a total past int64
	reqs[2].Commit, reqs[2].Vals = medianFixture([]int64{0, 1}, []int64{1 << 62, 1 << 62})
	// a commit paired with another set: no address matches, computed on the library's host route
	reqs[3].Commit, _ = medianFixture([]int64{0, 1, 2}, []int64{1, 1, 1})
	_, reqs[3].Vals = medianFixture([]int64{0}, []int64{7})
	reqs[3].Vals.Addresses[0] = 99
	want := []int{MedianZeroTime, MedianGoPath, MedianGoPath, MedianZeroTime}
	res, err := e.MedianTimes(reqs)
	if err != nil {
		t.Fatal(err)
	}
	for i := range res {
		if res[i].Code != want[i] {
			t.Fatalf("request %d: code %d, want %d", i, res[i].Code, want[i])
		}
	}
	if res[0].Seconds != -62135596800 || res[0].Nanos != 0 {
		t.Fatalf("zero time: %d.%09d", res[0].Seconds, res[0].Nanos)
	}
	if res[3].OnDevice || !res[0].OnDevice {
		t.Fatalf("routes: %v %v", res[0].OnDevice, res[3].OnDevice)
	}
}
