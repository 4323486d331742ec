/*
 * Adapter that registers the MI355X implementation of the LSOP08 codec (LsEncoder08 + LsDecoder08, the optimal
 * predictor over the 3 x 3 neighbourhood) under Gridfour's plug-in interface.
 *
 *   spec.addCompressionCodec("LSOP08", org.gridfour.hip.LsCodec08Hip.class, org.gridfour.hip.LsCodec08Hip.class);
 *
 * The packings are byte-identical to LsEncoder08's -- the Huffman container where its body is strictly shorter
 * than the Deflate one, else the Deflate container --, so files stay readable by stock Gridfour.  Public
 * no-argument constructor and both interfaces in the class's own implements clause, as CodecHolder and
 * addCompressionCodec require.  Not compiled in the build image (no JDK); see INTEGRATION.md.
 */
package org.gridfour.hip;

import java.io.IOException;
import java.io.PrintStream;
import org.gridfour.compress.ICompressionDecoder;
import org.gridfour.compress.ICompressionEncoder;
import org.gridfour.lsop.LsDecoder08;

public class LsCodec08Hip implements ICompressionEncoder, ICompressionDecoder {

  private final long handle = HipCodecNative.create(Integer.getInteger("gridfour.hip.device", 0));
  /** analysis statistics are host-side bookkeeping: delegate to the stock implementation */
  private final LsDecoder08 statsDelegate = new LsDecoder08();

  public LsCodec08Hip() {
  }

  @Override
  public byte[] encode(int codecIndex, int nRows, int nCols, int[] values) {
    return HipCodecNative.encode(handle, HipCodecNative.KIND_LSOP08, codecIndex, nRows, nCols, values);
  }

  @Override
  public int[] decode(int nRows, int nColumns, byte[] packing) throws IOException {
    return HipCodecNative.decode(handle, HipCodecNative.KIND_LSOP08, nRows, nColumns, packing);
  }

  @Override
  public byte[] encodeFloats(int codecIndex, int nRows, int nCols, float[] values) {
    return null;
  }

  @Override
  public float[] decodeFloats(int nRows, int nColumns, byte[] packing) throws IOException {
    return null;
  }

  @Override
  public boolean implementsFloatingPointEncoding() {
    return false;
  }

  @Override
  public boolean implementsIntegerEncoding() {
    return true;
  }

  @Override
  public void analyze(int nRows, int nColumns, byte[] packing) throws IOException {
    statsDelegate.analyze(nRows, nColumns, packing);
  }

  @Override
  public void reportAnalysisData(PrintStream ps, int nTilesInRaster) {
    statsDelegate.reportAnalysisData(ps, nTilesInRaster);
  }

  @Override
  public void clearAnalysisData() {
    statsDelegate.clearAnalysisData();
  }

  @Override
  protected void finalize() {
    HipCodecNative.destroy(handle);
  }
}
