'use strict';
// The engine loop with a denoised display (INTEGRATION.md, "Denoised display in the engine loop"):
// Update(), Render(), Denoise({temporal: true}) per tick on a NativeRenderer made with
// {frameColor: true} and SetPresentSource('denoised'); the camera yaws before every tick after the
// first and the frame count restarts, as the engine's onCameraMove does.  With `plain` the renderer
// gets no option beyond the pipeline and nothing but Update() + Render() is called.
//
// argv: JSON {sceneDir, width, height, pipeline, yaws: [deg...], plain, out}
// stdout: JSON {uniforms: [[33 words]...], puts: [{serial, width, height}]}; the bytes of put k go to
// `${out}.put.${k}` (every tick waits for its paint, so put k shows tick k).
const fs = require('fs');
const { NativeRenderer } = require('../../pathtracerdemo_amd/js/NativeRenderer');
const { loadCompiledScene } = require('../../pathtracerdemo_amd/js/scene_io');

class RecordingContext2D {
  constructor() { this.puts = []; this.renderer = null; }
  createImageData(w, h) { return { width: w, height: h, data: new Uint8ClampedArray(w * h * 4) }; }
  putImageData(img) {
    this.puts.push({ serial: this.renderer.PresentedSerial, width: img.width, height: img.height, data: Buffer.from(img.data) });
  }
}

async function main() {
  const req = JSON.parse(process.argv[2]);
  const canvas = { width: req.width, height: req.height };
  const ctx2d = new RecordingContext2D();
  canvas.getContext = (kind) => (kind === '2d' ? ctx2d : null);
  const options = req.plain ? { pipeline: req.pipeline, device: 0 } : { pipeline: req.pipeline, device: 0, frameColor: true };
  const renderer = new NativeRenderer(null, null, canvas, options);
  ctx2d.renderer = renderer;
  await renderer.Initialize(loadCompiledScene(req.sceneDir));
  if (!req.plain) renderer.SetPresentSource('denoised');
  const uniforms = [];
  for (let t = 0; t < req.yaws.length; t++) {
    if (t > 0 && req.yaws[t] !== req.yaws[t - 1]) {
      renderer.GetCamera().SetYaw(req.yaws[t]);
      renderer.ResetFrameCount();
    }
    renderer.Update();
    renderer.Render();
    if (!req.plain) renderer.Denoise({ temporal: true });
    uniforms.push(Array.from(renderer.Uniform));
    await renderer.PresentIdle();
    if (renderer.PresentError) throw renderer.PresentError;
  }
  const puts = ctx2d.puts.map((p, k) => {
    fs.writeFileSync(`${req.out}.put.${k}`, p.data);
    return { serial: p.serial, width: p.width, height: p.height };
  });
  renderer.Destroy();
  process.stdout.write(JSON.stringify({ uniforms, puts }));
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
